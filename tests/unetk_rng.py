"""The counter RNG of the library's dropout masks (csrc/common.h unetk_uniform), restated in numpy."""
import numpy as np


def fc_uniform_host(seed, idx):
    """unetk_uniform(seed, idx): murmur3 finaliser of (seed, element index) -> uniform [0, 1) (unetk_fc_fwd's mask, csrc/fc.hip)."""
    h = (idx.astype(np.uint64) * 0x9E3779B1 + seed) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return (h >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)


def unit_mask_host(seed, shape, keep):
    """The 0 | 1/keep mask the norm kernels regenerate: unetk_uniform(seed, flat NHWC element index) < keep."""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
    u = fc_uniform_host(seed & 0xFFFFFFFF, idx).reshape(shape)
    return np.where(u < np.float32(keep), np.float32(1.0 / keep), np.float32(0.0)).astype(np.float32)
