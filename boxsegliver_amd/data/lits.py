"""LiTS training input pipeline -- MI355X-first restatement of the reference's
DataLoader/Liver/input_pipeline.py (dataset collection :73-198, sampler `gen_train_batch` :285-378, per-sample processing
`data_processing_train` :243-284) and DataLoader/misc.py (`read_or_create_k_folds` :45-74).

On-disk format (the reference's own): `<root>/png/volume-<PID>/<slice:03d>_im.png` 16-bit grayscale = (HU clipped to
[-250, 300] + 250) * IM_SCALE (DataLoader/Liver/extract.py:32-35,72; the evaluation window [-200, 250] of input_pipeline.py:45-46
is the stored range [50, 500] * IM_SCALE), `<slice:03d>_lb.png` 8-bit = label * LB_SCALE (IM_SCALE = LB_SCALE = 64, :47-48);
`meta.json` (shipped with the reference: 131 cases) and `k_folds.txt` ("Fold i:pid pid ...").

Design: the reference feeds the GPU from tf.data CPU threads (PNG decode + crop + resize per sample per step).  An
MI355X has 288 GB of HBM and the whole decoded training set is ~35 GB as uint16, so `SliceStore` decodes every slice ONCE
and keeps it on the device; a step's batch is then the host-side sampler (a few hundred integer operations) + one gather
kernel (`unetk_lits_batch`).  Decoding: zlib inflate on host threads, the five PNG row filters undone on the device
(`unetk_png_unfilter`), pixels written straight into the resident store (the product needs neither cv2 nor PIL; the host-side
checker of that path, a pure-numpy PNG decoder, lives with the test infrastructure: `oracle/lits_ops.png_decode`, and both
halves are pinned by files a third-party encoder wrote: tests/golden/png/, made with Pillow).

The sampler restates the reference's selection logic literally (forced tumor / liver shares, crop placement around the
object box, random zoom and window level) on a `random.Random(seed)` / `numpy.random.RandomState(seed)` pair instead
of the reference's unseeded global generators.
"""
import copy
import json
import logging
import math
import random
import struct
import zlib
from pathlib import Path

import numpy as np
import torch

from ..utils import hostcpu

from .. import ops
from ..utils import distribution_utils

IM_SCALE = 64
LB_SCALE = 64
PNG_MAX_WIDTH = 4096           # csrc/lits.hip: unetk_png_unfilter keeps a band's carried row in LDS
LIVER_PERCENT = 0.66
TUMOR_PERCENT = 0.5
RND_SCALE = (1.0, 1.4)


def add_arguments(parser):
    """DataLoader/Liver/input_pipeline.py:54-70 (names / defaults verbatim) + --lits_root (where png/, meta.json and
    k_folds.txt live; the reference hard-codes <project>/data/LiTS)."""
    group = parser.add_argument_group(title="Input Pipeline Arguments")
    group.add_argument("--test_fold", type=int, default=2)
    group.add_argument("--im_height", type=int, default=256)
    group.add_argument("--im_width", type=int, default=256)
    group.add_argument("--im_channel", type=int, default=3)
    group.add_argument("--filter_size", type=int, default=0, help="Filter tumors small than the given size")
    group.add_argument("--noise_scale", type=float, default=0.1)
    group.add_argument("--zoom_scale", type=float, nargs=2, default=RND_SCALE)
    group.add_argument("--random_flip", type=int, default=1,
                       help="Random flip while training. 0 for no flip, 1 for flip only left/right, "
                            "2 for only up/down, 3 for left/right and up/down")
    group.add_argument("--eval_in_patches", action="store_true")
    group.add_argument("--eval_num_batches_per_epoch", type=int, default=100)
    group.add_argument("--eval_mirror", action="store_true")
    group.add_argument("--liver_percent", type=float, default=LIVER_PERCENT)
    group.add_argument("--tumor_percent", type=float, default=TUMOR_PERCENT)
    group.add_argument("--lits_root", type=str, default="data/LiTS")


# ------------------------------------------------------------------------------------------------- PNG codec
def png_inflate(data):
    """Host half of the loader: parse the chunks of a non-interlaced 8- / 16-bit grayscale PNG and inflate its IDAT stream.
    Returns (width, height, bit_depth, filtered) with `filtered` = uint8 [height * (1 + width * bit_depth / 8)]: per row one
    filter-type byte + the filtered scanline -- what `unetk_png_unfilter` turns into pixels on the device.  zlib.decompress
    releases the GIL, so a thread pool of these scales with the cores."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            break
    if hdr is None:
        raise ValueError("PNG without an IHDR chunk")
    w, h, depth, ctype, _, _, interlace = hdr
    if ctype != 0 or interlace != 0 or depth not in (8, 16):
        raise ValueError("only non-interlaced 8/16-bit grayscale PNGs are supported")
    raw = np.frombuffer(zlib.decompress(b"".join(idat) if len(idat) != 1 else idat[0]), dtype=np.uint8)
    if raw.size != h * (w * depth // 8 + 1):
        raise ValueError("PNG data stream has {} bytes, expected {}".format(raw.size, h * (w * depth // 8 + 1)))
    if w > PNG_MAX_WIDTH:
        raise ValueError("PNG is {} pixels wide; unetk_png_unfilter takes rows of at most {}".format(w, PNG_MAX_WIDTH))
    if h and int(raw[::w * depth // 8 + 1].max()) > 4:       # the device kernel's status word stays as the backstop
        raise ValueError("PNG row {} carries filter type {} (corrupt file)".format(
            int(np.argmax(raw[::w * depth // 8 + 1] > 4)), int(raw[::w * depth // 8 + 1].max())))
    return w, h, depth, raw


def png_filter_rows(arr, filters):
    """The FILTERED scanlines of `arr` (uint8 / uint16 [h, w]) with filter type filters[y % len(filters)] on row y -- the
    inverse of the five PNG un-filters, vectorised (filtering only needs the unfiltered neighbours).  uint8 [h, 1 + stride]."""
    arr = np.ascontiguousarray(arr)
    h, w = arr.shape
    bpp = 2 if arr.dtype == np.uint16 else 1
    rows = np.frombuffer(arr.astype(">u2").tobytes() if bpp == 2 else arr.astype(np.uint8).tobytes(), dtype=np.uint8)
    rows = rows.reshape(h, w * bpp).astype(np.int32)
    left = np.concatenate([np.zeros((h, bpp), np.int32), rows[:, :-bpp]], axis=1)                      # a
    up = np.concatenate([np.zeros((1, w * bpp), np.int32), rows[:-1]], axis=0)                         # b
    upleft = np.concatenate([np.zeros((h, bpp), np.int32), up[:, :-bpp]], axis=1)                      # c
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    preds = [np.zeros_like(rows), left, up, (left + up) >> 1, paeth]
    ft = np.array([int(filters[y % len(filters)]) for y in range(h)], dtype=np.int64)
    out = np.empty((h, 1 + w * bpp), dtype=np.uint8)
    out[:, 0] = ft
    for t in range(5):
        sel = ft == t
        out[sel, 1:] = ((rows[sel] - preds[t][sel]) & 255).astype(np.uint8)
    return out


def png_encode(arr, filters=None, level=6):
    """ndarray uint8 / uint16 [h, w] -> PNG bytes.  filters: None = type 0 on every row; else a sequence of filter types
    (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) applied cyclically per row -- libpng picks them adaptively, so real files mix
    all five (used to write synthetic datasets in tests / tools and by data/extract.py)."""
    arr = np.ascontiguousarray(arr)
    h, w = arr.shape
    depth = 16 if arr.dtype == np.uint16 else 8
    raw = png_filter_rows(arr, filters if filters is not None else (0,)).tobytes()

    def chunk(typ, payload):
        return struct.pack(">I", len(payload)) + typ + payload + struct.pack(">I", zlib.crc32(typ + payload) & 0xffffffff)

    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, 0, 0, 0, 0)) + \
        chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b"")


# ------------------------------------------------------------------------------------------------- dataset lists
def random_split_k_fold(items, k, seed=None):
    """DataLoader/misc.py:24-42: shuffle with NumPy's legacy generator seeded by `seed`, cut into k consecutive blocks of
    floor(n / k) items and deal the remainder one by one to the first folds (pinned on the reference's own output by
    tests/golden/ref_k_folds.json)."""
    items = list(items)
    np.random.RandomState(seed).shuffle(items)       # == np.random.seed(seed); np.random.shuffle(items), state untouched
    size = len(items) // k
    folds = [items[i * size:(i + 1) * size] for i in range(k)]
    for i, extra in enumerate(items[k * size:]):
        folds[i].append(extra)
    return folds


def read_or_create_k_folds(path, list_, k_split=None, seed=None):
    """DataLoader/misc.py:45-74: parse "Fold i:pid pid ..." lines, or create the split and write that file.  (The shipped
    data/LiTS/k_folds.txt is read as is; it was not produced by seed 1357 under today's NumPy.)"""
    path = Path(path)
    if path.exists():
        with path.open() as f:
            return [line[line.find(":") + 1:].strip().split(" ") for line in f.readlines()]
    if not isinstance(k_split, int) or k_split <= 0:
        raise ValueError("Wrong `k_split` value. Need a positive integer, got {}".format(k_split))
    k_folds = random_split_k_fold(list_, k_split, seed) if k_split > 1 else [list(list_)]
    with path.open("w") as f:
        for i, fold in enumerate(k_folds):
            f.write("Fold %d:" % i + " ".join(str(x) for x in fold) + "\n")
    return k_folds


def parse_case(case, filter_size=0):
    """input_pipeline.py:92-119: group the per-slice tumor boxes by slice, drop tumors not larger than filter_size."""
    case = copy.deepcopy(case)
    for k in ("tumors", "tumor_areas", "tumor_centers", "tumor_stddevs"):
        case.pop(k, None)
    ft = case.pop("tumor_slices_from_to")
    assert len(ft) == len(case["tumor_slices_index"]) + 1
    centers, stddevs = _maybe_json(case.pop("tumor_slices_centers")), _maybe_json(case.pop("tumor_slices_stddevs"))
    areas, coords = _maybe_json(case.pop("tumor_slices_areas")), _maybe_json(case.pop("tumor_slices"))
    case["centers"], case["stddevs"], case["slices"] = [], [], []
    slices = copy.deepcopy(case["tumor_slices_index"])
    for ii in range(len(ft) - 1):
        sel = [j for j, a in enumerate(areas[ft[ii]:ft[ii + 1]]) if a > filter_size]
        if not sel:
            case["tumor_slices_index"].remove(slices[ii])
        else:
            case["centers"].append([centers[ft[ii] + j] for j in sel])
            case["stddevs"].append([stddevs[ft[ii] + j] for j in sel])
            case["slices"].append([coords[ft[ii] + j] for j in sel])
    return case


def _maybe_json(v):
    return json.loads(v) if isinstance(v, str) else v      # the shipped meta.json stores the nested lists as strings


def collect_datasets(root, test_fold, mode, filter_tumor_size=0, filter_only_liver_in_val=True):
    """input_pipeline.py:73-198: meta.json + k_folds.txt -> the list of cases of `mode` ("train" / anything else = val)."""
    root = Path(root)
    with (root / "meta.json").open() as f:
        meta = {int(c["PID"]): c for c in json.load(f)}
    k_folds = read_or_create_k_folds(root / "k_folds.txt", sorted(meta), k_split=5, seed=1357)
    if test_fold + 1 > len(k_folds):
        raise ValueError("test_fold too large")
    test = k_folds[test_fold] if test_fold >= 0 else []
    train = [x for i, fold in enumerate(k_folds) if i != test_fold for x in fold]
    if mode == "train":
        return [parse_case(meta[i], filter_tumor_size) for i in sorted(int(x) for x in train)]
    val = [parse_case(meta[i], filter_tumor_size) for i in sorted(int(x) for x in test)]
    return [c for c in val if len(c["slices"]) > 0] if filter_only_liver_in_val else val


# ------------------------------------------------------------------------------------------------- resident slices
class SliceStore(object):
    """Every slice of the given cases decoded once and kept in device memory: `im` int16-typed storage of the uint16
    pixels [n_slices, h, w], `lb` uint8 [n_slices, h, w]; `offset[pid] + z` indexes slice z of case pid.

    Loading (round 4; the reference decodes per sample per step with cv2 on tf.data threads, input_pipeline.py:243-284):
    the store is allocated up front from meta.json's `size` fields; a thread pool reads the files and inflates their zlib
    streams (the GIL is released in both), `chunk` slices at a time, into one of two pinned staging buffers; each chunk is
    uploaded as FILTERED scanlines and `unetk_png_unfilter` writes the pixels straight into the store's slots while the
    pool already inflates the next chunk.  Peak host memory = the two staging buffers (2 x chunk x 0.77 MB at 512 x 512),
    whatever the dataset's size.  Under data parallelism (`strategy` with N > 1 replicas) each rank decodes its contiguous
    1/N share of the slices and the shares are broadcast rank by rank over the process group (RCCL / xGMI), so the node reads
    and inflates the dataset once, not N times."""

    def __init__(self, root, cases, device, strategy=None, chunk=256, threads=None):
        import concurrent.futures
        import os
        root = Path(root)
        self.device = device
        self.offset, files, n = {}, [], 0
        hw = None
        for case in cases:
            pid, depth = int(case["PID"]), int(case["size"][0])
            self.offset[pid] = n
            cur = (int(case["size"][1]), int(case["size"][2]))
            if hw is not None and cur != hw:
                raise ValueError("the resident store needs slices of one size, got {} and {}".format(hw, cur))
            hw = cur
            d = root / "png" / "volume-{:d}".format(pid)
            files.extend((d / "{:03d}_im.png".format(z), d / "{:03d}_lb.png".format(z)) for z in range(depth))
            n += depth
        if n == 0:
            raise ValueError("no slices to load")
        h, w = hw
        self.im = torch.empty((n, h, w), dtype=torch.int16, device=device)        # the uint16 pixels' bit patterns
        self.lb = torch.empty((n, h, w), dtype=torch.uint8, device=device)
        world = strategy.num_replicas_in_sync if strategy is not None else 1
        rank = strategy.rank if strategy is not None else 0
        share = [(n * r) // world for r in range(world + 1)]                       # rank r decodes slices [share[r], share[r + 1])
        lo, hi = share[rank], share[rank + 1]
        im_row, lb_row = h * (2 * w + 1), h * (w + 1)
        chunk = max(1, min(int(chunk), hi - lo))
        stage = [(torch.empty((chunk, im_row), dtype=torch.uint8).pin_memory() if device.type == "cuda" else torch.empty((chunk, im_row), dtype=torch.uint8),
                  torch.empty((chunk, lb_row), dtype=torch.uint8).pin_memory() if device.type == "cuda" else torch.empty((chunk, lb_row), dtype=torch.uint8))
                 for _ in range(2)]
        dev_stage = [(torch.empty((chunk, im_row), dtype=torch.uint8, device=device),
                      torch.empty((chunk, lb_row), dtype=torch.uint8, device=device)) for _ in range(2)]
        done = [None, None]                                                        # event: the device has consumed stage k
        status = torch.zeros(1, dtype=torch.int32, device=device)

        def inflate(slot, j, pair):
            for path, dst, depth_bits in ((pair[0], stage[slot][0], 16), (pair[1], stage[slot][1], 8)):
                try:
                    pw, ph, pd, raw = png_inflate(path.read_bytes())
                except (ValueError, zlib.error) as e:
                    raise ValueError("{}: {}".format(path, e))
                if (ph, pw, pd) != (h, w, depth_bits):
                    raise ValueError("{}: {}x{} {}-bit, expected {}x{} {}-bit".format(path, ph, pw, pd, h, w, depth_bits))
                dst[j].numpy()[:] = raw

        workers = int(threads or min(32, hostcpu.usable_cpus()))      # the cgroup's quota, not the host's count
        failure = None                     # a rank that cannot decode its share must not leave the others in the exchange below
        try:
            with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
                k = 0
                for c0 in range(lo, hi, chunk):
                    slot, cnt = k & 1, min(chunk, hi - c0)
                    if done[slot] is not None:
                        done[slot].synchronize()                                   # its previous upload has left the pinned buffer
                    for f in [pool.submit(inflate, slot, j, files[c0 + j]) for j in range(cnt)]:
                        f.result()
                    for which, depth_bits, dst in ((0, 16, self.im), (1, 8, self.lb)):
                        dev_stage[slot][which][:cnt].copy_(stage[slot][which][:cnt], non_blocking=True)
                        ops.png_unfilter(dev_stage[slot][which][:cnt], h, w, depth_bits, dst[c0:c0 + cnt], status)
                    if device.type == "cuda":
                        done[slot] = torch.cuda.Event()
                        done[slot].record()
                    k += 1
            if int(status.item()) != 0:
                raise ValueError("a PNG row carries an invalid filter type (corrupt file under {})".format(root / "png"))
        except (ValueError, OSError) as e:
            failure = e
        if world > 1:
            import torch.distributed as dist
            bad = torch.tensor([1 if failure is not None else 0], dtype=torch.int32, device=device)
            dist.all_reduce(bad, op=dist.ReduceOp.MAX)                             # everybody learns of a failure BEFORE the exchange
            if int(bad.item()) and failure is None:
                failure = ValueError("another rank could not decode its share of the slices under {}".format(root / "png"))
        if failure is not None:
            raise failure
        if world > 1:
            for r in range(world):                                                 # every rank's share to everyone (uneven shares: one broadcast each)
                if share[r + 1] > share[r]:
                    dist.broadcast(self.im[share[r]:share[r + 1]].view(torch.uint8), src=r)    # bytes: every backend moves uint8
                    dist.broadcast(self.lb[share[r]:share[r + 1]], src=r)
        self.load_stats = {"slices": n, "decoded_here": hi - lo, "chunk": chunk, "threads": workers,
                           "staging_bytes": 2 * chunk * (im_row + lb_row)}


# ------------------------------------------------------------------------------------------------- sampler
class TrainSampler(object):
    """Which slices, crops and windows make up a training batch -- the sampling POLICY of the reference's python generator
    (input_pipeline.py:285-378) as one vectorised draw per batch.

    The reference yields one sample at a time from nested Python loops and feeds it through tf.data's per-sample map.  Here
    the cases are flattened ONCE into numpy tables (volume extents, liver boxes, a CSR list of tumor slices and of the tumor
    boxes on each of them) and `draw()` emits the whole batch at once: the `[bs, C + 7]` int32 table + `[bs, 2]` windows
    that `unetk_lits_batch` consumes, with no per-sample Python.  The policy (not the random stream) is the reference's:
      * the first ceil(bs * tumor_percent) samples come from cases WITH tumors: a uniformly chosen tumor slice, the crop
        placed around a uniformly chosen tumor box of that slice; they also count as liver samples;
      * then, up to ceil(bs * liver_percent) samples in all, a uniformly chosen slice of the liver's z range, the crop
        placed around the liver box; the rest are uniformly chosen slices, crop anywhere;
      * crop extent = target size x U(random_scale) per axis; the crop's origin is uniform in the range that keeps the
        object box (shrunk by 5 px) inside the crop when that range is more than 20 px wide, else in
        [box start - 20, a point between the box's start and its centre] clipped to the image (:337-352);
      * neighbouring slices fill the other channels, -1 (zeros) outside the volume; window level uniform in
        [10, 50] / [500, 540] HU-units x IM_SCALE when random_window_level else fixed 50 / 500; independent flip coins.

    `guide` (a GuidePolicy) adds the spatial-guide objects of the guided pipeline (`guide_objects`); their draws come from
    a generator of their own, so a guided run draws the same slices, crops, windows and flips as an unguided one.
    `context` (bool): the context guide's coin (`guide_coin`) comes from that same generator, its --hist_noise normals from
    `noise_rng`, a sibling spawned from the same seed."""

    def __init__(self, data_list, batch_size, config, liver_percent=0., tumor_percent=0., random_scale=(1., 1.),
                 random_window_level=False, random_flip=0, seed=None, guide=None, context=False):
        self.bs, self.c = int(batch_size), int(config.im_channel)
        self.target = np.array([config.im_height, config.im_width], dtype=np.float64)
        self.scale = (float(random_scale[0]), float(random_scale[1]))
        self.window, self.flip = bool(random_window_level), int(random_flip or 0)
        self.rng = np.random.default_rng(seed)
        d = list(data_list)
        self.pid = np.array([int(c["PID"]) for c in d], dtype=np.int64)
        self.size = np.array([c["size"] for c in d], dtype=np.int64)                       # [n, (depth, H, W)]
        self.liver = np.array([c["bbox"] for c in d], dtype=np.int64)                      # [n, (z0, y0, x0, z1, y1, x1)]
        # CSR: case -> its tumor slices -> the tumor boxes (y0, x0, y1, x1) on each
        n_slices = np.array([len(c["slices"]) for c in d], dtype=np.int64)
        self.slice_ptr = np.concatenate(([0], np.cumsum(n_slices)))
        self.slice_z = np.array([z for c in d for z in c["tumor_slices_index"]], dtype=np.int64)
        n_boxes = np.array([len(bx) for c in d for bx in c["slices"]], dtype=np.int64)
        self.box_ptr = np.concatenate(([0], np.cumsum(n_boxes)))
        self.boxes = np.array([b for c in d for bx in c["slices"] for b in bx], dtype=np.int64).reshape(-1, 4)
        self.tumor_cases = np.flatnonzero(n_slices > 0)
        self.n_tumor = int(math.ceil(self.bs * tumor_percent))
        self.n_liver = max(int(math.ceil(self.bs * liver_percent)), self.n_tumor)          # tumor samples count as liver
        if self.n_tumor and len(self.tumor_cases) == 0:
            raise ValueError("tumor_percent > 0 needs at least one case with tumors")
        self.guide = guide
        if guide is not None or context:
            self.guide_rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(1)[0])
        if context:     # --hist_noise normals: a sibling of the guide generator, so the noise leaves the guides' draws alone
            self.noise_rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(2)[1])
        if guide is not None:
            self.moments = ObjectMoments(d, n_slices, self.slice_z, self.box_ptr)

    def _randint(self, lo, hi):
        """Uniform integers in [lo, hi] (inclusive, element-wise)."""
        if np.any(hi < lo):
            raise ValueError("empty crop range: the crop is larger than the slice")      # random.randint raises there
        return lo + np.floor(self.rng.random(lo.shape) * (hi - lo + 1)).astype(np.int64)

    def draw(self):
        """One batch: dict(case [bs] index into data_list, pid, z, chans [bs, C] (-1 = zeros), box [bs, 4] = (off_y, off_x,
        crop_h, crop_w), clip [bs, 2], flips [bs, 2], kind [bs] 0 tumor / 1 liver / 2 any)."""
        bs, rng = self.bs, self.rng
        j = np.arange(bs)
        kind = np.where(j < self.n_tumor, 0, np.where(j < self.n_liver, 1, 2))
        case = rng.integers(0, len(self.pid), bs)
        if self.n_tumor:
            case[:self.n_tumor] = self.tumor_cases[rng.integers(0, len(self.tumor_cases), self.n_tumor)]
        depth, h, w = self.size[case, 0], self.size[case, 1], self.size[case, 2]
        crop = np.floor(self.target[None, :] * rng.uniform(self.scale[0], self.scale[1], (bs, 2))).astype(np.int64)
        # the slice and the object box (y0, x0, y1, x1) the crop is placed around; "no object" = an inverted box
        z = np.floor(rng.random(bs) * depth).astype(np.int64)
        obj = np.stack([h, w, np.zeros_like(h), np.zeros_like(w)], axis=1)
        lv = kind == 1
        if lv.any():
            lb = self.liver[case[lv]]
            z[lv] = lb[:, 0] + np.floor(rng.random(int(lv.sum())) * (lb[:, 3] - lb[:, 0])).astype(np.int64)
            obj[lv] = lb[:, [1, 2, 4, 5]]
        tm = kind == 0
        if tm.any():
            ct = case[tm]
            s = self.slice_ptr[ct] + np.floor(rng.random(len(ct)) * (self.slice_ptr[ct + 1] - self.slice_ptr[ct])).astype(np.int64)
            z[tm] = self.slice_z[s]
            obj[tm] = self.boxes[self.box_ptr[s] + np.floor(rng.random(len(ct)) * (self.box_ptr[s + 1] - self.box_ptr[s])).astype(np.int64)]
        off = np.empty((bs, 2), dtype=np.int64)
        for ax, extent in ((0, h), (1, w)):
            start, stop, cr = obj[:, ax], obj[:, ax + 2], crop[:, ax]
            lo_in, hi_in = np.maximum(stop + 5 - cr, 0), np.minimum(start - 5, extent - cr)      # box (shrunk by 5) inside the crop
            wide = lo_in + 20 < hi_in
            anchor = np.floor(start * .75 + stop * .25).astype(np.int64) if ax == 0 else (start + stop) // 2
            lo = np.where(wide, lo_in, np.maximum(start - 20, 0))
            hi = np.where(wide, hi_in, np.minimum(anchor, extent - cr))
            off[:, ax] = self._randint(lo, hi)
        left = (self.c - 1) // 2
        chans = z[:, None] + np.arange(-left, self.c - left)[None, :]
        chans = np.where((chans >= 0) & (chans < depth[:, None]), chans, -1)
        if self.window:
            clip = np.stack([rng.integers(10, 51, bs), rng.integers(500, 541, bs)], axis=1).astype(np.float32) * IM_SCALE
        else:
            clip = np.tile(np.array([[50., 500.]], dtype=np.float32) * IM_SCALE, (bs, 1))
        flips = np.stack([(rng.random(bs) < 0.5) & bool(self.flip & 1), (rng.random(bs) < 0.5) & bool(self.flip & 2)], axis=1)
        return dict(case=case, pid=self.pid[case], z=z, chans=chans, box=np.concatenate([off, crop], axis=1), clip=clip,
                    flips=flips.astype(np.int32), kind=kind)

    def table(self, slice_offset, b=None):
        """The batch as `unetk_lits_batch` takes it: int32 [bs, C + 7] = (resident-store indices of the C channel slices, of
        the label slice, off_y, off_x, crop_h, crop_w, flip_lr, flip_ud), float32 [bs, 2] windows, int64 [bs] case ids.
        slice_offset: {pid: index of the case's first slice in the resident store}; b: a draw() (default: a new one)."""
        b = self.draw() if b is None else b
        base = np.array([slice_offset[int(p)] for p in b["pid"]], dtype=np.int64)
        tab = np.empty((self.bs, self.c + 7), dtype=np.int32)
        tab[:, :self.c] = np.where(b["chans"] >= 0, base[:, None] + b["chans"], -1)
        tab[:, self.c] = base + b["z"]
        tab[:, self.c + 1:self.c + 5] = b["box"]
        tab[:, self.c + 5:] = b["flips"]
        return tab, b["clip"], b["pid"]

    def guide_coin(self, spatial_random):
        """One guide coin per sample, random() < spatial_random (input_pipeline_g.py:528-529): the spatial guide and the
        context of a sample read the SAME coin, the first draw of the batch from `guide_rng`."""
        return self.guide_rng.random(self.bs) < spatial_random

    def guide_objects(self, b, coin=None):
        """The spatial-guide objects of the batch `b` (a draw()), gen_train_batch's policy (input_pipeline_g.py:527-599):
        a sample whose coin falls below spatial_random and whose slice is a tumour slice of its case keeps the tumours whose
        centre lies in the drawn crop (off <= c < off + crop on both axes); under inner_random a uniformly random non-empty
        subset of them of size randint(1, n) (the reference raises when none is in the box; that sample gets no guide
        here); then c' = c - off + s U(-r_c, r_c), s' = max(s U(1 / (1 + r_s), 1 + r_s), min_std), in float64 as the
        reference computes them.  Vectorised over the batch; the draws come from `guide_rng` alone.  coin: the batch's
        `guide_coin` when the context guide shares it (default: drawn here, the same first draw).
        Returns (obj_ptr int32 [bs + 1], obj float32 [M, 4] = (cy, cx, sy, sx)), centres relative to the crop."""
        g, rng, bs = self.guide, self.guide_rng, self.bs
        if coin is None:
            coin = self.guide_coin(g.spatial_random)
        ind = np.where(coin, self.moments.slice_index(b["case"], b["z"]), -1)
        ptr, c, s = self.moments.gather(ind)
        sample = np.repeat(np.arange(bs), np.diff(ptr))
        off, crop = b["box"][sample, :2], b["box"][sample, 2:]
        keep = np.all((off <= c) & (c < off + crop), axis=1)
        if g.inner_random:
            n_in = np.bincount(sample[keep], minlength=bs)
            k = 1 + np.floor(rng.random(bs) * n_in).astype(np.int64)                # randint(1, n_in); n_in = 0 keeps none
            key = np.where(keep, rng.random(len(sample)), np.inf)                  # a uniform order of each sample's in-box tumours
            order = np.lexsort((key, sample))
            rank = np.empty(len(sample), dtype=np.int64)
            rank[order] = np.arange(len(sample)) - ptr[sample[order]]
            keep &= rank < k[sample]
        sample, c, s, off = sample[keep], c[keep].astype(np.float64), s[keep].astype(np.float64), off[keep]
        rc, rs = float(g.center_ratio), float(g.stddev_ratio)
        c = s * rng.uniform(-rc, rc, c.shape) + (c - off)
        s = np.maximum(s * rng.uniform(1. / (1 + rs), 1. + rs, s.shape), float(g.min_std))
        obj_ptr = np.concatenate(([0], np.cumsum(np.bincount(sample, minlength=bs)))).astype(np.int32)
        return obj_ptr, np.concatenate([c, s], axis=1).astype(np.float32).reshape(-1, 4)


class GuidePolicy(object):
    """The spatial-guide knobs of gen_train_batch (input_pipeline_g.py:527-599): --spatial_random, --spatial_inner_random,
    --center_random_ratio, --stddev_random_ratio, --min_std (the sampler's stddev floor; the render floor is RENDER_MIN_STD)."""

    def __init__(self, spatial_random=1., inner_random=False, center_ratio=0.2, stddev_ratio=0.4, min_std=2.):
        self.spatial_random, self.inner_random = float(spatial_random), bool(inner_random)
        self.center_ratio, self.stddev_ratio, self.min_std = float(center_ratio), float(stddev_ratio), float(min_std)

    @classmethod
    def from_args(cls, args, spatial_random, inner_random):
        return cls(spatial_random, inner_random, getattr(args, "center_random_ratio", 0.2),
                   getattr(args, "stddev_random_ratio", 0.4), getattr(args, "min_std", 2.))


class ObjectMoments(object):
    """The tumours' centres (y, x) and stddevs of a case list as flat float32 tables in CSR over the tumour slices (the
    order of TrainSampler.boxes), and the reference's `tumor_slices_index.index(z)` as one searchsorted over (case, z)
    keys."""

    def __init__(self, cases, n_slices=None, slice_z=None, box_ptr=None):
        cases = list(cases)
        if n_slices is None:
            n_slices = np.array([len(c["slices"]) for c in cases], dtype=np.int64)
            slice_z = np.array([z for c in cases for z in c["tumor_slices_index"]], dtype=np.int64)
            n_boxes = np.array([len(bx) for c in cases for bx in c["slices"]], dtype=np.int64)
            box_ptr = np.concatenate(([0], np.cumsum(n_boxes)))
        self.box_ptr = box_ptr
        self.centers = np.array([p for c in cases for cs in c["centers"] for p in cs], dtype=np.float32).reshape(-1, 2)
        self.stddevs = np.array([p for c in cases for ss in c["stddevs"] for p in ss], dtype=np.float32).reshape(-1, 2)
        if not len(self.centers) == len(self.stddevs) == int(box_ptr[-1]):
            raise ValueError("tumour centres / stddevs do not match the tumour boxes of the cases")
        depth = max([int(c["size"][0]) for c in cases] + [int(slice_z.max(initial=-1)) + 1])
        self.span = depth + 1
        key = np.repeat(np.arange(len(cases)), n_slices) * self.span + slice_z
        self.order = np.argsort(key, kind="stable")            # sorted and unique in the shipped meta.json; first match wins
        self.key = key[self.order]

    def slice_index(self, case, z):
        """Tumour-slice index (into box_ptr) of slice z of case `case`, element-wise; -1 where z is no tumour slice."""
        case, z = np.asarray(case, dtype=np.int64), np.asarray(z, dtype=np.int64)
        if len(self.key) == 0:
            return np.full(case.shape, -1, dtype=np.int64)
        q = case * self.span + z
        pos = np.minimum(np.searchsorted(self.key, q), len(self.key) - 1)
        hit = (z >= 0) & (z < self.span) & (self.key[pos] == q)
        return np.where(hit, self.order[pos], -1)

    def gather(self, ind):
        """The tumours of the tumour slices `ind` (-1 = none): (ptr int64 [len(ind) + 1], centres, stddevs)."""
        ind = np.asarray(ind, dtype=np.int64)
        ind = np.where(ind < len(self.box_ptr) - 1, ind, -1)
        safe = np.maximum(ind, 0)
        bp = np.append(self.box_ptr, self.box_ptr[-1])                   # safe + 1 stays inside with no tumour slice at all
        cnt = np.where(ind >= 0, bp[safe + 1] - bp[safe], 0)
        ptr = np.concatenate(([0], np.cumsum(cnt))).astype(np.int64)
        idx = np.repeat(bp[safe] - ptr[:-1], cnt) + np.arange(ptr[-1])
        return ptr, self.centers[idx], self.stddevs[idx]


RENDER_MIN_STD = 1.0       # data_processing_train's kwargs.get("min_std", 1.): the flag never reaches it (input_pipeline_g.py:383)


def render_guide(tab, obj_ptr, obj, config, channels, src_hw):
    """sp_guide f32 [bs, H, W, 1] of a batch whose table `tab` is already on the device: obj_ptr / obj travel in ONE
    non-blocking copy from pinned memory (no host sync), then unetk_lits_spatial_guide on the current stream."""
    m = len(obj)
    host = torch.empty(4 * m + len(obj_ptr), dtype=torch.float32, pin_memory=True)
    host[:4 * m] = torch.from_numpy(obj.reshape(-1))
    host[4 * m:].view(torch.int32)[:] = torch.from_numpy(obj_ptr)
    dev = host.to(tab.device, non_blocking=True)
    return ops.lits_spatial_guide(tab, dev[4 * m:].view(torch.int32), dev[:4 * m].view(m, 4), (config.im_height, config.im_width),
                                  channels, src_hw, RENDER_MIN_STD)


CONTEXT_FEATURES = ("hist",)           # always served; `glcm` only with --glcm; the ct_conv context is not built
GLCM_LENGTH = 96                       # 8 properties x 3 distances x 4 angles (data/extract.py dump_glcm_feature)
GLCM_DEFAULTS = {"glcm_features": ["contrast", "dissimilarity", "homogeneity", "energy", "entropy", "correlation",
                                   "cluster_shade", "cluster_prominence"],
                 "glcm_distance": [1, 2, 3], "glcm_angle": [0., math.pi * 0.25, math.pi * 0.5, math.pi * 0.75]}


def parse_context_list(context_list, glcm=False):
    """--context_list name length [name length ...] -> [(name, length)] (input_pipeline_g.py:264-271).  `glcm` (--glcm): the
    co-occurrence texture rows are accepted too, 96 numbers per slice."""
    items = list(context_list or [])
    if not items:
        raise ValueError("--use_context needs --context_list, e.g. --context_list hist 200")
    if len(items) % 2 != 0:
        raise ValueError("context_list is not paired: {}".format(items))
    pairs = [(str(items[2 * i]), int(items[2 * i + 1])) for i in range(len(items) // 2)]
    for name, f_len in pairs:
        if name == "glcm" and glcm:
            if f_len != GLCM_LENGTH:
                raise ValueError("context feature `glcm` has {} numbers per slice, got length {}".format(GLCM_LENGTH, f_len))
        elif name == "glcm":
            raise ValueError("context feature `glcm` is not supported without --glcm; the LiTS pipeline builds {}".format(
                ", ".join(CONTEXT_FEATURES + ("glcm",))))
        elif name not in CONTEXT_FEATURES:
            raise ValueError("context feature `{}` is not supported; the LiTS pipeline builds {}".format(
                name, ", ".join(CONTEXT_FEATURES)))
    return pairs


_GLCM_NOISE_LOGGED = False


def context_list_from_args(args):
    """parse_context_list of the run's flags.  With --glcm the feature files hold the reference's one layout, so
    --glcm_features / --glcm_distance / --glcm_angle (commented out in the reference) must keep their defaults; --glcm_noise
    has no effect, as in the reference's LiTS pipeline (input_pipeline_g.py:276-291 fills the hist kwargs only)."""
    global _GLCM_NOISE_LOGGED
    glcm = bool(getattr(args, "glcm", False))
    if glcm:
        for flag, default in GLCM_DEFAULTS.items():
            value = getattr(args, flag, None)
            if value is not None and list(value) != default:
                raise ValueError("--{} {} is not supported: the glcm feature files hold {}".format(
                    flag, " ".join(str(v) for v in value), " ".join(str(v) for v in default)))
        if getattr(args, "glcm_noise", False) and not _GLCM_NOISE_LOGGED:
            _GLCM_NOISE_LOGGED = True
            logging.getLogger(__name__).warning("--glcm_noise has no effect: the LiTS pipeline adds noise to the hist columns only")
    return parse_context_list(getattr(args, "context_list", None), glcm=glcm)


def context_noise_scale(context_list, hist_noise_scale):
    """float64 [F]: the per-column scale of the training noise -- hist_noise_scale on `hist` columns, 0 on `glcm` columns."""
    return np.concatenate([np.full(n, float(hist_noise_scale) if name == "hist" else 0., dtype=np.float64)
                           for name, n in context_list])


def hist_preprocess(feat, hist_scale):
    """feature_ops.hist_preprocess: feat *= hist_scale (a float32 table times a Python float stays float32)."""
    return (feat * hist_scale).astype(np.float32)


def load_context_rows(lits_root, cases, offset, n_rows, context_list, mode_dir, hist_scale):
    """The host copy of the resident context table: float32 [n_rows, F] in SliceStore order (row offset[pid] + z), each
    case's <lits_root>/feat/<name>/<mode_dir>/<PID:03d>.npy preprocessed and concatenated over the context list
    (input_pipeline_g.py:531-543)."""
    feat_root = Path(lits_root) / "feat"
    width = sum(n for _, n in context_list)
    rows = np.zeros((n_rows, width), dtype=np.float32)
    for case in cases:
        pid, depth = int(case["PID"]), int(case["size"][0])
        col = 0
        for name, f_len in context_list:
            path = feat_root / name / mode_dir / "{:03d}.npy".format(pid)
            if not path.exists():
                raise FileNotFoundError("missing context features {}; make them with `python -m boxsegliver_amd.data.extract "
                                        "{} <dir of volume-*.nii> {}`".format(path, name, feat_root))
            feat = np.load(path, allow_pickle=False)
            if feat.ndim != 2 or feat.shape[1] != f_len:
                raise ValueError("{}: feature length mismatch {} vs {}".format(path, feat.shape[1:], f_len))
            if feat.shape[0] != depth:
                raise ValueError("{}: {} rows for a case of {} slices".format(path, feat.shape[0], depth))
            # feature_ops: hist_preprocess scales; glcm_preprocess is the cast alone (--hist_scale is for hist columns only)
            rows[offset[pid]:offset[pid] + depth, col:col + f_len] = \
                hist_preprocess(feat, hist_scale) if name == "hist" else feat.astype(np.float32)
            col += f_len
    return rows


class ContextGuide(object):
    """The context guide of one pipeline: the host copy of its table (load_context_rows), the coin's spatial_random and,
    in training with --hist_noise, the noise scale (a float, or a per-column float64 vector: context_noise_scale).
    `fresh(device)` uploads a new resident table -- one per generator,
    as the reference caches per generator -- which `unetk_lits_context` reads and, under noise, updates in place."""

    def __init__(self, rows, spatial_random=1., noise_scale=None):
        self.rows, self.spatial_random = rows, float(spatial_random)
        self.noise_scale = None if noise_scale is None else \
            (float(noise_scale) if np.ndim(noise_scale) == 0 else np.asarray(noise_scale, dtype=np.float64))

    def fresh(self, device):
        return torch.from_numpy(self.rows).to(device)


def upload_pinned(parts, device):
    """Numpy arrays -> device tensors in ONE non-blocking copy from pinned memory (no host sync); each part 16-byte aligned."""
    sizes, off = [], 0
    for a in parts:
        sizes.append(off)
        off += (a.nbytes + 15) & ~15
    host = torch.empty(max(off, 16), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for a, o in zip(parts, sizes):
        hv[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    dev = host.to(device, non_blocking=True)
    return [dev[o:o + a.nbytes].view(torch.from_numpy(a[:0]).dtype).view(a.shape) for a, o in zip(parts, sizes)]


def guides(tab_d, take, obj_ptr, obj, noise, table, config, channels, src_hw):
    """The guided batch's device work after one upload: (sp_guide or None, context)."""
    parts = [take.astype(np.int32)] + ([noise] if noise is not None else []) + \
        ([obj.reshape(-1, 4), obj_ptr] if obj is not None else [])
    dev = upload_pinned(parts, tab_d.device)
    take_d, rest = dev[0], dev[1:]
    noise_d = rest.pop(0) if noise is not None else None
    sp = None
    if obj is not None:
        sp = ops.lits_spatial_guide(tab_d, rest[1], rest[0], (config.im_height, config.im_width), channels, src_hw,
                                    RENDER_MIN_STD)
    return sp, ops.lits_context(table, tab_d, channels, take_d, noise_d)


def batches(store, data_list, config, training, seed=1234, liver_percent=0., tumor_percent=0., random_scale=(1., 1.),
            guide=None, context=None):
    """The tf.data pipelines get_dataset_for_train / get_dataset_for_eval_online (:381-430) as a generator of
    (features, labels) device batches: one vectorised sampler draw on the host, everything else in `unetk_lits_batch`.
    guide (a GuidePolicy): also features["sp_guide"] [bs, H, W, 1] (input_pipeline_g.py:382-412), rendered by
    `unetk_lits_spatial_guide` from the same device table, so it follows the image's crop and flips.
    context (a ContextGuide): also features["context"] [bs, F] (input_pipeline_g.py:527-550): the row of each sample's
    slice where its guide coin (shared with the spatial guide) succeeds, zeros elsewhere; with a noise scale, N(0, 1) x
    scale is added into the resident row first, so the noise builds up as in the reference.  Coin, guide objects and
    normals go up in one pinned copy."""
    bs = distribution_utils.per_device_batch_size(config.batch_size, config.num_gpus)
    c = config.im_channel
    sampler = TrainSampler(data_list, bs, config, liver_percent, tumor_percent, random_scale if training else (1., 1.),
                           random_window_level=training, random_flip=(getattr(config, "random_flip", 0) if training else 0),
                           seed=seed, guide=guide, context=context is not None)
    table = context.fresh(store.device) if context is not None else None
    step = 0
    while True:
        b = sampler.draw()
        tab, clip, names = sampler.table(store.offset, b)
        tab_d = torch.from_numpy(tab).to(store.device)
        images, labels = ops.lits_batch(store.im, store.lb, tab_d,
                                        torch.from_numpy(clip).to(store.device), (config.im_height, config.im_width), c,
                                        LB_SCALE, float(config.noise_scale) if training else 0.0, seed * 7919 + step)
        step += 1
        feats = {"images": images, "names": torch.from_numpy(names)}
        if context is not None:
            coin = sampler.guide_coin(context.spatial_random)
            obj_ptr, obj = sampler.guide_objects(b, coin) if guide is not None else (None, None)
            noise = None
            if training and context.noise_scale is not None:
                noise = sampler.noise_rng.normal(0., 1., (bs, table.shape[1])) * context.noise_scale
                if np.ndim(context.noise_scale) == 1:
                    noise[:, context.noise_scale == 0.] = -0.        # x + -0. keeps every bit of x, a row's -0. included
            sp, feats["context"] = guides(tab_d, coin, obj_ptr, obj, noise, table, config, c, store.im.shape[1:])
            if sp is not None:
                feats["sp_guide"] = sp
        elif guide is not None:
            obj_ptr, obj = sampler.guide_objects(b)
            feats["sp_guide"] = render_guide(tab_d, obj_ptr, obj, config, c, store.im.shape[1:])
        yield feats, labels


def batches_eval_3d(store, data_list, config, guide=None, context=None):
    """--eval_3d online evaluation (input_pipeline_g.py:602-700 `gen_eval_3d_online_batch` + :796-833): every validation
    case is served ONCE, as consecutive batch_size-slice batches over the liver's z range [z1, z2) -- the last batch padded
    with empty slices (index -1: zero image, zero label) -- each slice cropped to the liver box (y1, x1, y2 - y1, x2 - x1) and
    resized to the network size, fixed window, no noise, no flips; `names` carries the case id of the batch.
    The whole table of a case is laid out in one vectorised step; the gather kernel does the rest.
    guide (a GuidePolicy; only its min_std is used): also features["sp_guide"] with EVERY tumour of a tumour slice, centres
    relative to the liver box, stddevs max(s, min_std) -- no coin, no in-box filter, no perturbation (:679-690); 0.5 on
    the other slices and on padding.
    context (a ContextGuide of eval rows): also features["context"], the row of every slice, zeros on padding (:672-680)."""
    bs = distribution_utils.per_device_batch_size(config.batch_size, config.num_gpus)
    c = config.im_channel
    left = (c - 1) // 2
    ctx = np.arange(-left, c - left)[None, :]
    clip_row = np.array([[50., 500.]], dtype=np.float32) * IM_SCALE
    moments = ObjectMoments(data_list) if guide is not None else None
    table = context.fresh(store.device) if context is not None else None
    for ci, case in enumerate(data_list):
        z1, y1, x1, z2, y2, x2 = case["bbox"]
        depth, pid = case["size"][0], int(case["PID"])
        z = np.concatenate((np.arange(z1, z2), np.full((-(z2 - z1)) % bs, -100)))          # -100: padding (as the reference)
        chans = z[:, None] + ctx
        ok = (z[:, None] >= 0) & (chans >= 0) & (chans < depth)
        off = store.offset[pid]
        tab = np.zeros((len(z), c + 7), dtype=np.int32)
        tab[:, :c] = np.where(ok, off + chans, -1)
        tab[:, c] = np.where(z >= 0, off + z, -1)
        tab[:, c + 1:c + 5] = [y1, x1, y2 - y1, x2 - x1]
        if moments is not None:
            ptr, centers, stddevs = moments.gather(moments.slice_index(np.full(len(z), ci), z))
            obj = np.concatenate([centers - np.array([y1, x1], dtype=np.float32),
                                  np.maximum(stddevs, np.float32(guide.min_std))], axis=1).astype(np.float32)
        for b0 in range(0, len(z), bs):
            t = torch.from_numpy(np.ascontiguousarray(tab[b0:b0 + bs])).to(store.device)
            clip = torch.from_numpy(np.repeat(clip_row, bs, axis=0)).to(store.device)
            images, labels = ops.lits_batch(store.im, store.lb, t, clip, (config.im_height, config.im_width), c, LB_SCALE, 0.0, 0)
            feats = {"images": images, "names": torch.full((bs,), pid, dtype=torch.int64)}
            if context is not None:
                p = ptr[b0:b0 + bs + 1] if moments is not None else None
                sp, feats["context"] = guides(t, np.ones(bs, dtype=np.int32), None if p is None else (p - p[0]).astype(np.int32),
                                              None if p is None else obj[p[0]:p[-1]], None, table, config, c,
                                              store.im.shape[1:])
                if sp is not None:
                    feats["sp_guide"] = sp
            elif moments is not None:
                p = ptr[b0:b0 + bs + 1]
                feats["sp_guide"] = render_guide(t, (p - p[0]).astype(np.int32), obj[p[0]:p[-1]], config, c, store.im.shape[1:])
            yield feats, labels


def input_fn(mode, params):
    """input_pipeline.py:199-241 for the modes train / eval_online; params["lits_root"] holds png/, meta.json,
    k_folds.txt.  Offline volume evaluation: `input_fn_eval` below."""
    args = params["args"]
    root = params["lits_root"]
    device = params.get("device", torch.device("cuda", torch.cuda.current_device()))
    key = ("lits_store", mode == "train")
    if key not in params:
        cases = collect_datasets(root, args.test_fold, "train" if mode == "train" else "val",
                                 filter_tumor_size=getattr(args, "filter_size", 0))
        params[key] = (SliceStore(root, cases, device, strategy=params.get("strategy")), cases)
    store, cases = params[key]
    if len(cases) == 0:
        raise ValueError("No valid dataset found!")
    rs = tuple(getattr(args, "zoom_scale", (1., 1.)))                        # --zoom_scale (input_pipeline.py:62)
    base_seed = int(getattr(args, "seed", 1234) or 1234)
    seed = base_seed + 1000 * int(params.get("rank", 0))                     # training: every replica its own shard of the stream
    guided = bool(getattr(args, "use_spatial", False))
    use_context = bool(getattr(args, "use_context", False))
    sr = float(getattr(args, "spatial_random", 1.))
    if guided:
        # the guided pipeline (input_pipeline_g.py:282-301): the module's own forced shares, one guide channel
        if int(getattr(args, "guide_channel", 1)) != 1:
            raise ValueError("the LiTS spatial guide has one channel, got --guide_channel {}".format(args.guide_channel))
        train_guide = GuidePolicy.from_args(args, sr, getattr(args, "spatial_inner_random", False))
        eval_guide = GuidePolicy.from_args(args, 0. if sr < 1. else sr, False)
    else:
        train_guide = eval_guide = None
    if guided or use_context:
        liver_percent, tumor_percent = LIVER_PERCENT, TUMOR_PERCENT
    else:
        liver_percent, tumor_percent = getattr(args, "liver_percent", 0.), getattr(args, "tumor_percent", 0.)
    context = None
    if use_context:
        # the context table: train rows for training, eval rows for both eval_online modes (input_pipeline_g.py:734, :815)
        context_list = context_list_from_args(args)
        hist_scale = float(getattr(args, "hist_scale", 20.))
        ckey = ("lits_context", mode == "train", tuple(context_list), hist_scale)
        if ckey not in params:
            params[ckey] = load_context_rows(root, cases, store.offset, store.im.shape[0], context_list,
                                             "train" if mode == "train" else "eval", hist_scale)
        rows = params[ckey]
        if mode == "train":
            noise = float(getattr(args, "hist_noise_scale", 0.002)) if getattr(args, "hist_noise", False) else None
            if noise is not None and any(name != "hist" for name, _ in context_list):
                noise = context_noise_scale(context_list, noise)
            context = ContextGuide(rows, sr, noise)
        else:
            context = ContextGuide(rows, 0. if sr < 1. else sr)
    if mode == "train":
        return batches(store, cases, args, True, seed, liver_percent, tumor_percent, rs, guide=train_guide, context=context)
    if mode == "eval_online" and getattr(args, "eval_3d", False):
        return batches_eval_3d(store, cases, args, guide=eval_guide, context=context)
    if mode == "eval_online":
        # rank-INDEPENDENT stream: the reference (one process) evaluates one sample, and the evaluator hooks let rank 0 alone
        # decide / save -- every replica must see the same validation data so their best-result state stays identical
        gen = batches(store, cases, args, False, base_seed + 500, liver_percent, tumor_percent, guide=eval_guide,
                      context=context)
        n = int(getattr(args, "eval_num_batches_per_epoch", 100))
        return (next(gen) for _ in range(n))
    raise ValueError("lits.input_fn handles the modes `train` and `eval_online`, got {}".format(mode))


def input_fn_eval(mode, params):
    """input_pipeline.py:228-234 for ModeKeys.EVAL / PREDICT: a python generator over the NIfTI volumes of the validation
    fold (paths in meta.json's vol_case / lab_case, relative to params["proj_root"]).  The evaluator uploads each slab and
    does mirroring / accumulation / argmax on the GPU (evaluators/evaluator_liver.py); with --use_context (without
    --use_spatial) each case's eval context rows are uploaded once here and the slabs carry device views of them.
    params["volumes_on"] == "device": each case's raw crop is uploaded once and the slabs are built on the device
    (_device_slabs); --eval_in_patches keeps the host generator."""
    args = params["args"]
    cases = collect_datasets(params["lits_root"], args.test_fold, mode, filter_tumor_size=getattr(args, "filter_size", 0),
                             filter_only_liver_in_val=params.get("filter_only_liver_in_val", True))
    if len(cases) == 0:
        raise ValueError("No valid dataset found!")
    proj_root = params.get("proj_root", ".")
    context = None
    if getattr(args, "use_context", False) and not getattr(args, "use_spatial", False):
        # input_pipeline_g.py:910-980 (get_dataset_for_eval_image): every slab carries its slices' eval context rows
        context = EvalContext(params["lits_root"], context_list_from_args(args),
                              float(getattr(args, "hist_scale", 20.)), params.get("device"))
    fixed = None
    if getattr(args, "use_spatial", False) and getattr(args, "eval_no_sp", False):
        fixed = eval_no_sp_features(args, params.get("device"))
    if getattr(args, "eval_in_patches", False):
        if context is not None or fixed is not None:
            raise ValueError("--eval_in_patches does not serve the context or spatial guide")
        return get_dataset_for_eval_patches(cases, config=args, proj_root=proj_root)
    device = None
    if params.get("volumes_on") == "device":
        device = params.get("device") or torch.device("cuda", torch.cuda.current_device())
    if params.get("whole_slices", False):
        return get_dataset_for_eval_image(cases, args, proj_root, context=context, fixed=fixed, device=device)
    return get_dataset_for_eval_image_v2(cases, args, proj_root, context=context, fixed=fixed, device=device)


def eval_no_sp_features(args, device=None):
    """--use_spatial --eval_no_sp (input_pipeline_g.py:982-1050, get_dataset_for_eval_image_sp): every slab carries
    sp_guide = 0.5 everywhere and, with --use_context, a context of zeros -- constant device tensors made once.  The
    reference's --real_sp meta guides in these slabs, --save_sp_guide and --mode infer are not supported."""
    if getattr(args, "real_sp", None):
        raise NotImplementedError("--real_sp guides in the --eval_no_sp slabs are not supported")
    if getattr(args, "save_sp_guide", False):
        raise NotImplementedError("--save_sp_guide is not supported with --eval_no_sp")
    if getattr(args, "mode", "eval") == "infer":
        raise NotImplementedError("--mode infer with --use_spatial --eval_no_sp is not supported")
    device = device or torch.device("cuda", torch.cuda.current_device())
    bs = int(args.batch_size)
    fixed = {"sp_guide": torch.full((bs, int(args.im_height), int(args.im_width), 1), 0.5, dtype=torch.float32,
                                    device=device)}
    if getattr(args, "use_context", False):
        width = sum(n for _, n in context_list_from_args(args))
        fixed["context"] = torch.zeros((bs, width), dtype=torch.float32, device=device)
    return fixed


class EvalContext(object):
    """The eval context rows of the offline evaluators: `case(case, pads)` loads a case's rows (load_context_rows,
    <lits_root>/feat/<name>/eval/), appends `pads` zero rows at the end of the whole volume as the reference does, and
    uploads them ONCE; the slabs then carry device views of it."""

    def __init__(self, lits_root, context_list, hist_scale, device=None):
        self.root, self.context_list, self.hist_scale = lits_root, context_list, hist_scale
        self.device = device or torch.device("cuda", torch.cuda.current_device())

    def case(self, case, pads):
        depth = int(case["size"][0])
        rows = load_context_rows(self.root, [case], {int(case["PID"]): 0}, depth, self.context_list, "eval", self.hist_scale)
        rows = np.concatenate((rows, np.zeros((pads, rows.shape[1]), rows.dtype)), axis=0)
        return torch.from_numpy(rows).to(self.device)


def slab_context_rows(z0, n, batch_size):
    """input_pipeline_g.py:966-969: the slab starting at centre slice z0 + idx reads context_val[sid:sid + batch_size] with
    sid = z0 + idx, for idx = 0, batch_size, ... < n (z0: the first evaluated slice of the volume)."""
    return [(z0 + idx, z0 + idx + batch_size) for idx in range(0, n, batch_size)]


# ------------------------------------------------------------------------------------------------- offline evaluation
GRAY_MIN, GRAY_MAX = -200, 250       # input_pipeline.py:45-46


def cv2_linear_taps(dst_n, src_n):
    """One axis of cv2_resize_linear: (i0, i1, f) per destination sample -- it reads src[i0] * (1 - f) + src[i1] * f.
    (Also the tap arrays of the device slab builder, ops.eval_slab.)"""
    s = (np.arange(dst_n, dtype=np.float64) + 0.5) * (src_n / float(dst_n)) - 0.5
    i0 = np.floor(s).astype(np.int64)
    f = (s - i0).astype(np.float32)
    lo = i0 < 0
    i0[lo], f[lo] = 0, 0.0
    hi = i0 >= src_n - 1
    i0[hi], f[hi] = src_n - 1, 0.0
    return i0, np.minimum(i0 + 1, src_n - 1), f


def cv2_resize_linear(img, dsize):
    """cv2.resize(img, dsize, interpolation=cv2.INTER_LINEAR) for float arrays [H, W] or [H, W, C]; dsize = (width, height).
    OpenCV's rule: source coordinate (dst + 0.5) * (src / dst) - 0.5, taps clamped to the image (border replicate)."""
    dw, dh = int(dsize[0]), int(dsize[1])
    img = np.asarray(img, np.float32)
    sh, sw = img.shape[:2]
    if (sh, sw) == (dh, dw):
        return img.copy()
    y0, y1, fy = cv2_linear_taps(dh, sh)
    x0, x1, fx = cv2_linear_taps(dw, sw)
    ex = (Ellipsis,) if img.ndim == 2 else (Ellipsis, None)
    rows = img[y0] * (1.0 - fy)[(slice(None), None) + ((None,) if img.ndim == 3 else ())] + \
        img[y1] * fy[(slice(None), None) + ((None,) if img.ndim == 3 else ())]
    fxb = fx[(None, slice(None)) + ((None,) if img.ndim == 3 else ())]
    del ex
    return (rows[:, x0] * (1.0 - fxb) + rows[:, x1] * fxb).astype(np.float32)


def _grown_span(lo, hi, pad, extent, align, at_least=0):
    """One axis of the evaluation window: the object's half-open span [lo, hi) grown by `pad`, clipped to [0, extent),
    widened to `at_least` pixels if shorter, then its length rounded UP to a multiple of `align` about the same centre.
    Returns (start, stop, wanted length); stop - start < wanted length when the far border clipped it."""
    a, b = max(lo - pad, 0), min(hi + pad, extent)
    if at_least:
        if at_least > extent:
            raise ValueError("Cannot satisfied conditions!")
        if b - a < at_least:
            a = min(max(a - (at_least - (b - a)) // 2, 0), extent - at_least)
            b = a + at_least
    want = -(-(b - a) // align) * align
    start = max(int((a + b - 1) / 2 - (want - 1) / 2), 0)
    return start, min(start + want, extent), want


def aligned_window(case, align, padding, min_shape=None):
    """The (y, x) window of a case that the evaluators cut from every slice: the liver box + `padding`, at least `min_shape`,
    sides rounded up to `align` (input_pipeline.py:444-479,556-580).  When the far border clips EITHER axis so that its
    side is no longer a multiple of `align`, BOTH axes are re-anchored at their far ends (the reference's rule; it warns
    when that pushes a start below zero).  Returns (y1, y2, x1, x2)."""
    _, h, w = case["size"]
    bb = case["bbox"]
    spans = [_grown_span(bb[1], bb[4], padding, h, align, min_shape[0] if min_shape else 0),
             _grown_span(bb[2], bb[5], padding, w, align, min_shape[1] if min_shape else 0)]
    if any((stop - start) % align for start, stop, _ in spans):
        spans = [(stop - want, stop, want) for _, stop, want in spans]
        if any(start < 0 for start, _, _ in spans):
            print("\nWarning: bbox aligns with {} failed! point1 ({}, {}) point2 ({}, {})\n".format(
                align, spans[1][0], spans[0][0], spans[1][1], spans[0][1]))
    return spans[0][0], spans[0][1], spans[1][0], spans[1][1]


def _load_lits_volume(case, root, test_data=False):
    from . import nii_kits
    obj_num = int(case["vol_case"][:-4].split("-")[-1])
    if test_data:
        return obj_num, nii_kits.read_nii(root / case["vol_case"])[1]
    return obj_num, nii_kits.read_lits(obj_num, "vol", root / case["vol_case"])[1]


def _window_normalise(volume):
    """HU window [GRAY_MIN, GRAY_MAX] -> [0, 1], (z, y, x) -> (y, x, z) float32 (input_pipeline.py:595-596)."""
    volume = (np.clip(volume, GRAY_MIN, GRAY_MAX) - GRAY_MIN) / (GRAY_MAX - GRAY_MIN)
    return volume.transpose((1, 2, 0)).astype(np.float32)


def _case_eval_crop(case, align, padding, padding_z, im_channel, parse_label=True, test_data=False, proj_root="."):
    """The raw part of parse_case_eval: the int16 HU crop [z, y, x] of the liver box with the context slices the volume
    has, and (before, after) = the context slices beyond it, which parse_case_eval pads with HU 0 before the window."""
    from . import nii_kits
    d, h, w = case["size"]
    z1, z2 = max(case["bbox"][0] - padding_z, 0), min(case["bbox"][3] + padding_z, d)
    y1, y2, x1, x2 = aligned_window(case, align, padding)
    root = Path(proj_root)
    obj_num, volume = _load_lits_volume(case, root, test_data)
    lhc = (im_channel - 1) // 2                       # context slices before / after the centre slice of a sample
    rhc = im_channel - 1 - lhc
    lo, hi = z1 - lhc, z2 + rhc                       # zero slices stand in for context beyond the volume
    crop = volume[max(lo, 0):min(hi, d), y1:y2, x1:x2]
    segmentation, lab_case = None, None
    if parse_label:
        _, segmentation = nii_kits.read_lits(obj_num, "lab", root / case["lab_case"])
        segmentation = segmentation.astype(np.uint8)[z1:z2, y1:y2, x1:x2]
        lab_case = case["lab_case"]
    bbox = [x1, y1, z1, x2 - 1, y2 - 1, z2 - 1]
    return case["PID"], case["vol_case"], lab_case, bbox, [d, h, w], lhc, rhc, crop, (max(-lo, 0), max(hi - d, 0)), segmentation


def parse_case_eval(case, align, padding, padding_z, im_channel, parse_label=True, test_data=False, proj_root="."):
    """input_pipeline.py:556-612: the liver box (+ padding, sides rounded up to `align`) of one NIfTI case ->
    normalised float32 volume (y, x, z) with the half-channel context slices, cropped uint8 segmentation (z, y, x)."""
    pid, vol_case, lab_case, bbox, size, lhc, rhc, crop, beyond, segmentation = _case_eval_crop(
        case, align, padding, padding_z, im_channel, parse_label, test_data, proj_root)
    volume = np.pad(crop, (beyond, (0, 0), (0, 0)))
    cshape = list(volume.shape)
    volume = _window_normalise(volume)
    return pid, vol_case, lab_case, bbox, size, cshape, lhc, rhc, volume, segmentation


def _mirrored(eval_batch, config):
    """The mirrored copies of a slab under --eval_mirror (input_pipeline.py:538-553): variant 1 = flipped along W when
    random_flip has bit 0, 2 = along H with bit 1, 3 = both -- the last one whenever `random_flip & 3 > 0`, i.e. also for
    random_flip 1 and 2 (the reference's test, kept literally; evaluators.mirror_plan averages accordingly)."""
    if not getattr(config, "eval_mirror", False):
        return
    rf = int(config.random_flip)
    for variant, wanted, axes in ((1, rf & 1, (2,)), (2, rf & 2, (1,)), (3, rf & 3, (1, 2))):
        if wanted > 0:
            yield dict(eval_batch, images=np.flip(eval_batch["images"], axis=axes), mirror=variant), None


def _slabs(volume, batch_size, lhc, rhc, head, config, context=None, z0=0):
    """Serve a (y, x, z) volume as batch_size-slice slabs with (lhc, rhc) context slices per sample, each followed by its
    mirrored copies.  `head` = the constant entries of every slab's feature dict.  context (a device tensor of the case's
    rows): every slab -- and its mirrored copies, unflipped -- also carries context[sid:sid + batch_size] of
    slab_context_rows(z0, ...)."""
    n = volume.shape[-1] - lhc - rhc
    assert n % batch_size == 0, "Wrong padding"
    win = np.lib.stride_tricks.sliding_window_view(volume, lhc + rhc + 1, axis=-1)      # [y, x, n, c] without copying
    rows = slab_context_rows(z0, n, batch_size)
    for k, idx in enumerate(range(0, n, batch_size)):
        slab = dict(head, images=np.ascontiguousarray(np.moveaxis(win[:, :, idx:idx + batch_size], 2, 0)), mirror=0)
        if context is not None:
            slab["context"] = context[rows[k][0]:rows[k][1]]
        yield slab, None
        for item in _mirrored(slab, config):
            yield item


def window_table():
    """f32 [GRAY_MAX - GRAY_MIN + 1]: _window_normalise of every integer HU value of the window, by the host's own
    expression -- the device slab builder (ops.eval_slab) clamps into the window and reads this table."""
    return _window_normalise(np.arange(GRAY_MIN, GRAY_MAX + 1).reshape(-1, 1, 1)).reshape(-1)


def _device_slabs(crop, planes, out_hw, batch_size, c, head, device, context=None, z0=0):
    """_slabs on the device: `crop` (raw int16 HU [z, y, x]) is uploaded once, and every slab's images are built there by
    ops.eval_slab -- window, bilinear resize to out_hw = (rows, columns) and the channel window in one launch, bit-equal to
    the host's _window_normalise / cv2_resize_linear / _slabs.  planes int32 [n + c - 1]: what the host's padded volume
    holds at each z: a slice of `crop`, -1 = zeros added after the window, -2 = HU 0 padded before it.  One more small
    upload carries every table of the case.  No mirrored copies and no "mirror" key: the evaluator mirrors on the device."""
    if crop.dtype != np.int16:
        raise ValueError("the device slab builder takes int16 HU volumes, got {}".format(crop.dtype))
    n = len(planes) - (c - 1)
    assert n % batch_size == 0, "Wrong padding"
    zsrc = np.lib.stride_tricks.sliding_window_view(np.asarray(planes, np.int32), c)          # [n, c]
    taps_y, taps_x = cv2_linear_taps(out_hw[0], crop.shape[1]), cv2_linear_taps(out_hw[1], crop.shape[2])
    ints = [zsrc.reshape(-1), taps_y[0], taps_y[1], taps_x[0], taps_x[1]]
    floats = [taps_y[2], taps_x[2], window_table()]
    parts = [np.asarray(a, np.int32) for a in ints] + [np.asarray(a, np.float32).view(np.int32) for a in floats]
    packed = torch.from_numpy(np.concatenate(parts)).to(device)                                # one upload: every table
    views, pos = [], 0
    for a in parts:
        views.append(packed[pos:pos + a.size])
        pos += a.size
    zs, y0, y1, x0, x1 = views[:5]
    fy, fx, lut = (v.view(torch.float32) for v in views[5:])
    vol = torch.from_numpy(np.ascontiguousarray(crop)).to(device)                              # one upload: the HU crop
    rows = slab_context_rows(z0, n, batch_size)
    for k, idx in enumerate(range(0, n, batch_size)):
        images = ops.eval_slab(vol, zs[idx * c:(idx + batch_size) * c].view(batch_size, c), (y0, y1, fy), (x0, x1, fx), lut,
                               out_hw, c, window=(GRAY_MIN, GRAY_MAX))
        slab = dict(head, images=images)
        if context is not None:
            slab["context"] = context[rows[k][0]:rows[k][1]]
        yield slab, None


def get_dataset_for_eval_image_v2(data_list, config, proj_root=".", context=None, fixed=None, device=None):
    """input_pipeline.py:615-668: per case the liver box is cut from the NIfTI volume, padded in z to whole batches,
    resized to the network size, and served as batch_size-slice slabs (each followed by its mirrored copies under
    --eval_mirror); a case ends with (None, (segmentation, vol_path, pads, bbox, resize)).  context (an EvalContext):
    every slab also carries its slices' eval context rows as a device tensor (input_pipeline_g.py:910-980).  fixed: entries
    every slab carries unchanged (eval_no_sp_features).  device (a torch device): the raw crop is uploaded once per case and
    the slabs' images are device tensors built there (_device_slabs), without mirrored copies; the rest of the stream is
    the same."""
    align = 16 if getattr(config, "model", "UNet") != "DenseUNet" else 32
    padding, padding_z = 25, 0
    batch_size = config.batch_size
    c = config.im_channel
    pshape = config.im_height, config.im_width
    resize = not (config.im_height <= 0 or config.im_width <= 0)
    parse_label = getattr(config, "mode", "eval") != "infer"
    for case in data_list[getattr(config, "eval_skip_num", 0):]:
        if device is not None:
            pid, vol_path, _, bbox, _, lhc, rhc, crop, beyond, segmentation = _case_eval_crop(
                case, align, padding, padding_z, c, parse_label=parse_label, proj_root=proj_root)
            pads = -(bbox[5] - bbox[2] + 1) % batch_size
            planes = [-2] * beyond[0] + list(range(crop.shape[0])) + [-2] * beyond[1] + [-1] * pads
            out_hw = (pshape[1], pshape[0]) if resize else crop.shape[1:]     # cv2's dsize is (width, height)
            ctx = context.case(case, pads) if context is not None else None
            for item in _device_slabs(crop, planes, out_hw, batch_size, c, dict(fixed or {}, names=pid), device, ctx, bbox[2]):
                yield item
            yield None, (segmentation, vol_path, pads, bbox, resize)
            continue
        pid, vol_path, _, bbox, _, cshape, lhc, rhc, volume, segmentation = parse_case_eval(
            case, align, padding, padding_z, c, parse_label=parse_label, proj_root=proj_root)
        if not resize:
            pshape = tuple(cshape[1:])
        pads = -(bbox[5] - bbox[2] + 1) % batch_size          # zero slices that complete the last slab
        volume = np.pad(volume, ((0, 0), (0, 0), (0, pads)))
        if resize:
            volume = cv2_resize_linear(volume, pshape)      # dsize = (im_height, im_width), as the reference passes it
        ctx = context.case(case, pads) if context is not None else None
        for item in _slabs(volume, batch_size, lhc, rhc, dict(fixed or {}, names=pid), config, ctx, bbox[2]):
            yield item
        yield None, (segmentation, vol_path, pads, bbox, resize)


def get_dataset_for_eval_image(data_list, config, proj_root=".", test_data=False, context=None, fixed=None, device=None):
    """input_pipeline_li.py:398-456: whole slices (no liver crop); context, fixed and device as in
    get_dataset_for_eval_image_v2."""
    from . import nii_kits
    batch_size = config.batch_size
    c = config.im_channel
    pshape = config.im_height, config.im_width
    resize = not (config.im_height <= 0 or config.im_width <= 0)
    root = Path(proj_root)
    parse_label = getattr(config, "mode", "eval") != "infer"
    lhc = (c - 1) // 2
    rhc = c - 1 - lhc
    for case in data_list[getattr(config, "eval_skip_num", 0):]:
        obj_num, volume = _load_lits_volume(case, root, test_data)
        raw = volume
        if device is None:
            volume = _window_normalise(volume)
        segmentation, seg_path = None, None
        if parse_label:
            _, segmentation = nii_kits.read_lits(obj_num, "lab", root / case["lab_case"])
            segmentation, seg_path = segmentation.astype(np.uint8), case["lab_case"]
        ori_d, h, w = raw.shape
        pads = -ori_d % batch_size
        ctx = context.case(case, pads) if context is not None else None
        head = dict(fixed or {}, names=case["PID"])
        if device is not None:
            planes = [-1] * lhc + list(range(ori_d)) + [-1] * (pads + rhc)
            out_hw = (pshape[1], pshape[0]) if resize else (h, w)
            for item in _device_slabs(raw, planes, out_hw, batch_size, c, head, device, ctx, 0):
                yield item
        else:
            volume = np.pad(volume, ((0, 0), (0, 0), (lhc, pads + rhc)))       # context + the zero slices of the last slab
            if resize:
                volume = cv2_resize_linear(volume, pshape)
            for item in _slabs(volume, batch_size, lhc, rhc, head, config, ctx, 0):
                yield item
        yield None, (segmentation, seg_path, pads, (0, 0, 0, w - 1, h - 1, ori_d - 1), resize)


def parse_case_patches(case, align, padding, padding_z, min_shape=None):
    """input_pipeline.py:444-479: the liver box (+ padding) grown to at least `min_shape` (the patch) inside the slice,
    then its sides rounded up to `align` around the centre."""
    d, h, w = case["size"]
    z1, z2 = max(case["bbox"][0] - padding_z, 0), min(case["bbox"][3] + padding_z, d)
    y1, y2, x1, x2 = aligned_window(case, align, padding, min_shape)
    return case["PID"], d, h, w, z1, y1, x1, z2, y2, x2


def patch_centres(extent, psize, step=2):
    """input_pipeline.py:725-731 along one axis: window centres from psize/2 to extent - psize/2 in equal steps of at most
    psize/step, rounded -- the windows tile [0, extent) with overlap, first and last flush with the borders."""
    start, end = psize // 2, extent - psize // 2
    num = math.ceil((end - start) / (psize / step))
    size = (end - start) / (num + 1e-8)
    if size == 0:
        size = 9999999
    return np.round(np.arange(start, end + 1e-8, size)).astype(np.int32)


def get_dataset_for_eval_patches(data_list, step=2, config=None, proj_root="."):
    """--eval_in_patches, input_pipeline.py:676-766: the liver box of each case is evaluated at NATIVE resolution by
    sliding an (im_height, im_width) window over every slice (window stride <= patch / step), batched batch_size windows
    at a time.  Yields (eval_batch, None) ... and, with the case's last batch, (eval_batch, labels) -- the whole label
    volume (z, y, x); eval_batch = {images [bs, ph, pw, c], name, pad, bbox, position[(z, lb_y, ub_y, lb_x, ub_x)]}.
    The reference indexes x windows with the patch HEIGHT (:743-744); identical for the square patches it is used with,
    restated here with the width."""
    import itertools
    from . import nii_kits
    align, padding, padding_z = 16, 25, 0
    batch_size = config.batch_size
    c = config.im_channel
    psize = int(config.im_height), int(config.im_width)
    root = Path(proj_root)
    for case in data_list[getattr(config, "eval_skip_num", 0):]:
        pid, d, h, w, z1, y1, x1, z2, y2, x2 = parse_case_patches(case, align, padding, padding_z, min_shape=psize)
        obj_num = int(case["vol_case"][:-4].split("-")[-1])
        _, volume = nii_kits.read_lits(obj_num, "vol", root / case["vol_case"])
        lhc = (c - 1) // 2
        rhc = c - 1 - lhc
        left_pad = lhc - z1 if z1 < lhc else 0
        right_pad = z2 + rhc - d if z2 + rhc > d else 0
        volume = volume[max(0, z1 - lhc):min(d, z2 + rhc), y1:y2, x1:x2]
        cd, ch, cw = volume.shape
        if left_pad > 0 or right_pad > 0:
            volume = np.concatenate((np.zeros((left_pad, ch, cw), dtype=volume.dtype), volume,
                                     np.zeros((right_pad, ch, cw), dtype=volume.dtype)), axis=0)
            cd, ch, cw = volume.shape
        volume = (np.clip(volume, GRAY_MIN, GRAY_MAX) - GRAY_MIN) / (GRAY_MAX - GRAY_MIN)
        volume = volume.transpose((1, 2, 0)).astype(np.float32)     # (y, x, z)
        ysteps, xsteps = patch_centres(ch, psize[0], step), patch_centres(cw, psize[1], step)
        all_patches = list(itertools.product(xsteps, ysteps, range(lhc, cd - rhc)))
        num_of_batches = (len(all_patches) + (batch_size - 1)) // batch_size
        for batch in range(num_of_batches):
            eval_batch = {"images": np.zeros((batch_size,) + psize + (c,), dtype=np.float32), "name": pid, "pad": 0,
                          "bbox": [x1, y1, z1, x2 - 1, y2 - 1, z2 - 1], "position": [None] * batch_size}
            chunk = all_patches[batch * batch_size:(batch + 1) * batch_size]
            for i, (x, y, z) in enumerate(chunk):
                lb_y, ub_y = y - psize[0] // 2, y + psize[0] // 2
                lb_x, ub_x = x - psize[1] // 2, x + psize[1] // 2
                eval_batch["images"][i] = volume[lb_y:ub_y, lb_x:ub_x, z - lhc:z + rhc + 1]
                eval_batch["position"][i] = (z - lhc, lb_y, ub_y, lb_x, ub_x)
            if batch < num_of_batches - 1:
                yield eval_batch, None
            else:
                eval_batch["pad"] = batch_size - len(chunk)
                _, labels = nii_kits.read_lits(obj_num, "lab", root / case["lab_case"])
                yield eval_batch, labels
