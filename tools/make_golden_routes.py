"""Generate ``tests/golden/g6_routes.npz`` by running the REAL reference on CPU (golden generation only).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_routes.py

Needs the reference tree (imported unmodified through ``oracle/_refshim.py``); the tests only read the ``.npz``.
Records:
  * ``cross_scan_fn`` / ``cross_merge_fn`` (CrossScanF / CrossMergeF, models/csm_triton.py:22-273) forward and backward
    for every (in_channel_first, out_channel_first, one_by_one, scans in 0/1/2) the torch path computes, on two odd
    rectangular shapes.  Two configurations of the torch path's one_by_one scan (``cross_scan1b1_fwd``) slip, and the
    Triton kernel this project follows does not: channel-last scans=2 indexes ``x[:, k]`` on the H axis instead of the
    route axis (:119-124), and channel-first scans=1 flattens (C, H) instead of (H, W) (``x.flatten(2, 3)``, :99), which
    is only harmless when the output stays channel-first.  Neither the scan of those configurations nor the merge whose
    backward is that scan is recorded.
  * SS2Dv2(d_model=16, d_state=1, channel_first=True) for ``v051d_noz`` / ``v052d_noz`` (fusion_vmamba.py:977-978) at
    (2,16,7,7) and (1,16,6,10), recorded like the G4 ``ss2dv2`` entries (oracle/make_golden.py).
"""
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _refshim  # noqa: E402
from oracle.make_golden import _block_record, _np  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g6_routes.npz")
SHAPES = (("a", (2, 3, 5, 7)), ("b", (1, 4, 6, 9)))
CONFIGS = list(itertools.product((True, False), (True, False), (False, True), (0, 1, 2)))


def torch_slip(in_cf, out_cf, obo, scans):
    """The configurations whose torch one_by_one scan differs from triton_cross_scan_flex (see the module docstring)."""
    return obo and (((not in_cf) and scans == 2) or (in_cf and not out_cf and scans == 1))


def config_tag(in_cf, out_cf, obo, scans):
    return f"{int(in_cf)}{int(out_cf)}{int(obo)}{scans}"


def x_shape(B, C, H, W, in_cf, obo):
    if obo:
        return (B, 4, C, H, W) if in_cf else (B, H, W, 4, C)
    return (B, C, H, W) if in_cf else (B, H, W, C)


def y_shape(B, C, H, W, out_cf):
    return (B, 4, C, H, W) if out_cf else (B, H, W, 4, C)


def gen_routes(ct, store):
    for name, (B, C, H, W) in SHAPES:
        for cfg in CONFIGS:
            in_cf, out_cf, obo, scans = cfg
            if torch_slip(in_cf, out_cf, obo, scans):
                continue
            tag = f"{name}/{config_tag(*cfg)}"
            g = torch.Generator().manual_seed(11)
            x = torch.randn(*x_shape(B, C, H, W, in_cf, obo), generator=g).requires_grad_()
            y = ct.cross_scan_fn(x, in_cf, out_cf, obo, scans)
            gy = torch.randn(*y.shape, generator=g)
            y.backward(gy)
            yin = torch.randn(*y_shape(B, C, H, W, out_cf), generator=g).requires_grad_()
            m = ct.cross_merge_fn(yin, in_cf, out_cf, obo, scans)
            gm = torch.randn(*m.shape, generator=g)
            m.backward(gm)
            for k, v in dict(x=x, scan=y, gscan=gy, dx=x.grad, yin=yin, merge=m, gmerge=gm, dyin=yin.grad).items():
                store[f"{tag}/{k}"] = _np(v)
    print("g6 routes", len(store), "arrays")


def gen_blocks(fv, store):
    g = torch.Generator().manual_seed(6)
    for ft in ("v051d_noz", "v052d_noz"):
        torch.manual_seed(6)
        m = fv.SS2Dv2(d_model=16, d_state=1, ssm_ratio=1.0, dt_rank="auto", conv_bias=False, forward_type=ft,
                      channel_first=True)
        _block_record(store, f"{ft}/a", m, [torch.randn(2, 16, 7, 7, generator=g)], False)
        m = fv.SS2Dv2(d_model=16, d_state=1, ssm_ratio=2.0, dt_rank="auto", conv_bias=False, forward_type=ft,
                      channel_first=True)
        _block_record(store, f"{ft}/b", m, [torch.randn(1, 16, 6, 10, generator=g)], False)


def main():
    _, ct, fv, _ = _refshim.load()
    store = {}
    gen_routes(ct, store)
    gen_blocks(fv, store)
    np.savez_compressed(OUT, **store)


if __name__ == "__main__":
    main()
