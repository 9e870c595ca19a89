"""Records what `liver_3d` uploads per batch WITHOUT --random_rotate: tests/golden/lits3d_rotate_off.npz.

Run once, at the commit before the flag existed:  python tests/golden/make_lits3d_rotate_fixtures.py
test_lits3d_rotate_host.py imports `stream` from here and holds the pipeline with the feature off to the recorded tables:
the rotation draw may not move any other draw of the generator.

`stream` drives the real generator, data/lits3d.batches, on the synthetic cases of lits3d_ref.make_cases() with the device
calls replaced by recorders, so it needs no GPU: the sample tables, and with a guide the click tables, as they are uploaded."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

import lits3d_ref as ref  # noqa: E402

OUT = os.path.join(HERE, "lits3d_rotate_off.npz")
N_TABLES = 3
SHAPE = (6, 16, 20)
CONFIGS = {"unguided": None, "guided": dict(channels=2, stddev=None)}


def sampler(bs=2, tumor_percent=0.5, seed=1234, random_flip=7, fg=2, **kw):
    from boxsegliver_amd.data import lits3d
    cases = ref.make_cases()
    _, lb, base = ref.stack_store(cases)
    counts = (lb // 64 >= fg).sum(axis=(1, 2))
    meta = [{"PID": pid, "size": [im.shape[0], ref.H, ref.W]} for pid, (im, _) in enumerate(cases)]
    offset = {pid: int(b) for pid, b in enumerate(base)}
    return lits3d.PatchSampler(meta, offset, counts, bs, SHAPE, (ref.H, ref.W), tumor_percent=tumor_percent, seed=seed,
                               random_flip=random_flip, **kw)


class _FakeStore(object):
    device = torch.device("cpu")

    def __init__(self):
        self.im = torch.zeros((sum(ref.DEPTHS), ref.H, ref.W), dtype=torch.int16)
        self.lb = torch.zeros((sum(ref.DEPTHS), ref.H, ref.W), dtype=torch.uint8)


def stream(guide, n=N_TABLES, **kw):
    """(sample tables int32 [n, bs, 16], click tables int32 [n, bs, 12] or None, the keywords every wrapper call got) of the
    first n batches of data/lits3d.batches; kw: the sampler's."""
    from boxsegliver_amd.data import lits, lits3d
    tabs, ctabs, calls = [], [], []

    def upload(parts, device):
        tabs.append(parts[0].copy())
        if len(parts) > 1:
            ctabs.append(parts[1].copy())
        return [torch.from_numpy(p.copy()) for p in parts]

    def recorder(name, result):
        def call(*a, **k):
            calls.append((name, dict(k)))
            return result
        return call
    one = torch.zeros(1)
    stubs = [(lits, "upload_pinned", upload), (lits3d.ops, "lits_pick_voxels", recorder("lits_pick_voxels", None)),
             (lits3d.ops, "lits_patch3d", recorder("lits_patch3d", (one, one))),
             (lits3d.ops, "lits3d_clicks", recorder("lits3d_clicks", (one, one))),
             (lits3d.ops, "click_guide3d", recorder("click_guide3d", one))]
    saved = [(mod, name, getattr(mod, name)) for mod, name, _ in stubs]
    try:
        for mod, name, fn in stubs:
            setattr(mod, name, fn)
        gen = lits3d.batches(_FakeStore(), sampler(**kw), SHAPE, 2, 2, torch.zeros(1, dtype=torch.int32), guide)
        for _ in range(n):
            next(gen)
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)
    return np.stack(tabs), (np.stack(ctabs) if ctabs else None), calls


def main():
    out = {}
    for name, guide in CONFIGS.items():
        tabs, ctabs, _ = stream(guide)
        out[name + "_tab"] = tabs
        if ctabs is not None:
            out[name + "_clicks"] = ctabs
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
