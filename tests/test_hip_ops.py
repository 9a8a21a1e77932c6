"""GPU parity tests of the operator boundary: the HIP kernels
behind the C ABI vs (i) golden vectors recorded from the real reference and (ii) the CPU oracle on
seeded inputs.  Tolerances are BASELINE.json's: 1e-3 (fp32 I/O) / 1e-2 (16-bit I/O), relative to
the tensor's magnitude."""
import os

import numpy as np
import pytest
import torch

from oracle import c_scan
from oracle import xfm_oracle as O
from oracle.golden_inputs import G1_CASES
from tests.helpers import assert_close, g1_case_tensors, load_npz

pytestmark = pytest.mark.gpu
GRADS = ("u", "delta", "A", "B", "C", "D", "delta_bias")
DEV = "cuda"


def _tol(dtype):
    return 1e-3 if dtype == torch.float32 else 1e-2


def _run_hip(t, softplus, oflex=True):
    import xfmamba_amd
    leaves = {k: (t[k].to(DEV).requires_grad_() if t[k] is not None else None) for k in GRADS}
    y = xfmamba_amd.selective_scan_fn(leaves["u"], leaves["delta"], leaves["A"], leaves["B"], leaves["C"],
                                      leaves["D"], leaves["delta_bias"], softplus, oflex)
    y.backward(t["dout"].to(DEV).to(y.dtype))
    torch.cuda.synchronize()
    return y.detach().cpu(), {k: (v.grad.detach().cpu() if v is not None else None) for k, v in leaves.items()}


def _check(y, grads, y_ref, g_ref, tol):
    assert_close(y.float(), y_ref, tol, tol * float(y_ref.abs().max()), "y")
    for k in GRADS:
        if g_ref.get(k) is None:
            assert grads[k] is None
            continue
        ref = g_ref[k].float()
        assert_close(grads[k].float(), ref, tol, tol * (float(ref.abs().max()) + 1e-6), "d" + k)


@pytest.mark.parametrize("case", G1_CASES, ids=[c[0] for c in G1_CASES])
def test_selective_scan_matches_reference_golden(case):
    z = load_npz("g1_scan.npz")
    name = case[0]
    t = g1_case_tensors(z, case)
    y, grads = _run_hip(t, case[7])
    assert y.dtype == torch.float32                      # oflex
    g_ref = {k: (torch.from_numpy(z[f"{name}/d{k}"]) if f"{name}/d{k}" in z.files else None) for k in GRADS}
    _check(y, grads, torch.from_numpy(z[f"{name}/y"]), g_ref, _tol(t["u"].dtype))
    for k in ("u", "delta", "B", "C"):
        assert grads[k].dtype == t[k].dtype


SHAPES = [
    # (B, K, Dg, N, L, dtype)   hot-path shaped, shrunk in batch/width (SURVEY 8(a) call table)
    (2, 4, 96, 1, 3136, torch.float32),     # stage 0
    (2, 4, 192, 1, 784, torch.bfloat16),    # stage 1
    (3, 4, 384, 1, 196, torch.float32),     # stage 2
    (4, 4, 768, 1, 49, torch.bfloat16),     # stage 3
    (2, 2, 1536, 16, 49, torch.float32),    # shallow fusion
    (2, 4, 1536, 16, 49, torch.bfloat16),   # deep fusion
    (1, 4, 128, 1, 9216, torch.float32),    # XFMamba-B @384 stage 0
    (1, 4, 64, 16, 144, torch.float16),     # XFMamba-B @384 fusion
    (2, 1, 24, 8, 4096, torch.float32),     # reference test shape (test_selective_scan.py:153-156), long row, few rows
    (2, 2, 12, 8, 1134, torch.bfloat16),    # ragged length from the reference's seqlen list
    (1, 1, 1, 1, 1, torch.float32),         # degenerate
    (1, 3, 5, 3, 7, torch.float32),         # odd everything (tile = 1 row)
    (2, 1, 8, 64, 33, torch.float32),       # wide state
]


def _rand_inputs(shape, seed):
    Bt, K, Dg, N, L, dt = shape
    g = torch.Generator().manual_seed(seed)
    KD = K * Dg
    t = dict(u=torch.randn(Bt, KD, L, generator=g), delta=0.5 * torch.rand(Bt, KD, L, generator=g),
             A=-0.5 * torch.rand(KD, N, generator=g) - 0.05, B=torch.randn(Bt, K, N, L, generator=g),
             C=torch.randn(Bt, K, N, L, generator=g), D=torch.randn(KD, generator=g),
             delta_bias=0.5 * torch.rand(KD, generator=g), dout=torch.randn(Bt, KD, L, generator=g))
    for k in ("u", "delta", "B", "C"):
        t[k] = t[k].to(dt)
    return t


@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{s[0]}K{s[1]}D{s[2]}N{s[3]}L{s[4]}{str(s[5])[6:]}" for s in SHAPES])
def test_selective_scan_matches_oracle(shape):
    t = _rand_inputs(shape, seed=11)
    y, grads = _run_hip(t, True)
    y_ref = c_scan.scan_fwd_c(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["delta_bias"], True)
    g = c_scan.scan_bwd_c(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["delta_bias"], t["dout"], True)
    _check(y, grads, y_ref, dict(zip(GRADS, g)), _tol(shape[5]))


def test_selective_scan_options_and_strides():
    import xfmamba_amd
    t = _rand_inputs((2, 2, 16, 4, 100, torch.float32), seed=5)
    # no D, no bias, no softplus, oflex False on bf16, non-contiguous batch/row strides
    big_u = torch.randn(2, 40, 100, device=DEV)
    u = big_u[:, 4:36]                                       # row stride 100, batch stride 4000, offset
    delta = (0.3 * torch.rand(2, 32, 100, device=DEV))
    A = t["A"].to(DEV)
    Bm, Cm = t["B"].to(DEV), t["C"].to(DEV)
    y = xfmamba_amd.selective_scan_fn(u, delta, A, Bm, Cm, None, None, False, True)
    y_ref = c_scan.scan_fwd_c(u.cpu(), delta.cpu(), t["A"], t["B"], t["C"], None, None, False)
    assert_close(y.cpu(), y_ref, 1e-3, 1e-3 * float(y_ref.abs().max()), "strided/no-softplus")
    ub, db, Bb, Cb = (v.to(torch.bfloat16) for v in (u.contiguous(), delta, Bm, Cm))
    yb = xfmamba_amd.selective_scan_fn(ub, db, A, Bb, Cb, t["D"].to(DEV), None, True, False)
    assert yb.dtype == torch.bfloat16
    yb_ref = c_scan.scan_fwd_c(ub.cpu(), db.cpu(), t["A"], Bb.cpu(), Cb.cpu(), t["D"], None, True)
    assert_close(yb.float().cpu(), yb_ref, 1e-2, 1e-2 * float(yb_ref.abs().max()), "bf16 out")
    with pytest.raises(RuntimeError):
        xfmamba_amd.selective_scan_fn(ub, delta, A, Bb, Cb)   # mixed dtypes are rejected, like the reference FFI


def test_selective_scan_full_size_properties():
    """BASELINE config-1 size (batch 64 = 32 x 2 views, stage-0 shape): size-independent properties.
    (a) linearity in u for fixed delta; (b) D-only path: with B = 0 the output is exactly D*u;
    (c) batch independence: row results equal those of the same rows scanned alone."""
    import xfmamba_amd
    torch.manual_seed(0)
    Bt, K, Dg, N, L = 64, 4, 96, 1, 3136
    KD = K * Dg
    dt = torch.bfloat16
    u1 = torch.randn(Bt, KD, L, device=DEV, dtype=dt)
    delta = (0.5 * torch.rand(Bt, KD, L, device=DEV)).to(dt)
    A = -torch.ones(KD, N, device=DEV)
    Bm = torch.randn(Bt, K, N, L, device=DEV, dtype=dt)
    Cm = torch.randn(Bt, K, N, L, device=DEV, dtype=dt)
    D = torch.randn(KD, device=DEV)
    bias = 0.1 * torch.rand(KD, device=DEV)
    f = lambda u, B_: xfmamba_amd.selective_scan_fn(u, delta, A, B_, Cm, D, bias, True, True)
    y1 = f(u1, Bm)
    y2 = f(u1 * 2, Bm)                                       # exact in bf16: doubling is lossless
    assert_close(y2, 2 * y1, 1e-4, 1e-4 * float(y1.abs().max()), "linearity")
    y0 = f(u1, torch.zeros_like(Bm))
    assert_close(y0, D[None, :, None] * u1.float(), 1e-6, 1e-6, "D path")
    sub = xfmamba_amd.selective_scan_fn(u1[5:6], delta[5:6], A, Bm[5:6], Cm[5:6], D, bias, True, True)
    # a batch of 1 gets a different work decomposition (lanes per row), so equality holds to rounding only
    assert_close(sub, y1[5:6], 1e-5, 1e-5 * float(y1.abs().max()), "batch independence")
    yc = c_scan.scan_fwd_c(u1[5:6, :8].cpu(), delta[5:6, :8].cpu(), A[:8].cpu(), Bm[5:6, :1].cpu(), Cm[5:6, :1].cpu(),
                           D[:8].cpu(), bias[:8].cpu(), True)
    assert_close(y1[5:6, :8].cpu(), yc, 1e-2, 1e-2 * float(yc.abs().max()), "spot rows vs oracle")


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 4, 12, 12), (2, 96, 56, 56), (3, 40, 7, 7), (1, 5, 96, 96),
                                   (2, 7, 14, 9)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_scan_merge_bit_exact_and_adjoint(shape, dtype):
    import xfmamba_amd
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g).to(dtype)
    Bt, C, H, W = shape
    xd = x.to(DEV).requires_grad_()
    ys = xfmamba_amd.cross_scan_fn(xd)
    assert torch.equal(ys.cpu(), O.cross_scan_ref(x))                     # pure data movement: bit-exact
    gy = torch.randn(Bt, 4, C, H * W, generator=g).to(dtype)
    ys.backward(gy.to(DEV))
    ref = O.cross_merge_ref(gy.float().view(Bt, 4, C, H, W)).view(Bt, C, H, W)
    assert_close(xd.grad.float().cpu(), ref, _tol(dtype), 1e-5, "scan backward = merge")
    yin = torch.randn(Bt, 4, C, H, W, generator=g)                        # merge consumes the fp32 scan output
    yd = yin.to(DEV).requires_grad_()
    m = xfmamba_amd.cross_merge_fn(yd)
    assert_close(m.cpu(), O.cross_merge_ref(yin), 1e-6, 1e-6, "merge")
    gm = torch.randn(Bt, C, H * W, generator=g)
    m.backward(gm.to(DEV))
    assert torch.equal(yd.grad.cpu(), O.cross_scan_ref(gm.view(Bt, C, H, W)).view(Bt, 4, C, H, W))


def test_cross_scan_merge_golden():
    import xfmamba_amd
    z = load_npz("g2_cross.npz")
    for n in ("a", "b"):
        x = torch.from_numpy(z[f"{n}/x"]).to(DEV)
        assert torch.equal(xfmamba_amd.cross_scan_fn(x).cpu(), torch.from_numpy(z[f"{n}/scan"]))
        yin = torch.from_numpy(z[f"{n}/yin"]).to(DEV)
        assert_close(xfmamba_amd.cross_merge_fn(yin).cpu(), torch.from_numpy(z[f"{n}/merge"]), 1e-6, 1e-6)


def test_swap_golden_and_passthrough_backward():
    import xfmamba_amd
    z = load_npz("g3_swap.npz")
    x = torch.from_numpy(z["x"]).to(DEV).requires_grad_()
    x2 = torch.from_numpy(z["x2"]).to(DEV).requires_grad_()
    xs = xfmamba_amd.SwappingScan_multiview.apply(x, x2)
    assert torch.equal(xs.cpu(), torch.from_numpy(z["swap"]))
    xs.backward(torch.from_numpy(z["gswap"]).to(DEV))
    assert torch.equal(x.grad.cpu(), torch.from_numpy(z["dx"])) and torch.equal(x2.grad.cpu(), torch.from_numpy(z["dx2"]))
    ys = torch.from_numpy(z["ys"]).to(DEV).requires_grad_()
    o1, o2 = xfmamba_amd.SwappingMerge_multiview.apply(ys)
    assert torch.equal(o1.cpu(), torch.from_numpy(z["o1"])) and torch.equal(o2.cpu(), torch.from_numpy(z["o2"]))
    torch.autograd.backward([o1, o2], [torch.from_numpy(z["g1"]).to(DEV), torch.from_numpy(z["g2"]).to(DEV)])
    assert torch.equal(ys.grad.cpu(), torch.from_numpy(z["dys"]))
    xb = torch.randn(3, 10, 4, 5, device=DEV, dtype=torch.bfloat16)
    xb2 = torch.randn(3, 10, 4, 5, device=DEV, dtype=torch.bfloat16)
    assert torch.equal(xfmamba_amd.SwappingScan_multiview.apply(xb, xb2).cpu(), O.swap_scan_ref(xb.cpu(), xb2.cpu()))


@pytest.mark.parametrize("shape", [(2, 96, 56, 56), (2, 192, 28, 28), (3, 40, 14, 14), (5, 33, 7, 7), (1, 6, 96, 96),
                                   (2, 5, 9, 13), (2, 64, 48, 48), (3, 128, 24, 24), (2, 36, 12, 12), (5, 256, 12, 12)])   # 6-vector rows (384^2 inputs)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("has_bias", [False, True])
def test_dwconv3x3_silu_matches_torch_fp32(shape, dtype, has_bias):
    """Row a4/a8/a9 front end: act(conv2d(x)) with nn.Conv2d(D,D,3,padding=1,groups=D) + nn.SiLU
    (reference fusion_vmamba.py:1198-1201).  Checker: the same op in plain PyTorch fp32 on CPU."""
    from xfmamba_amd.dwconv import dwconv3x3_silu_fn
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(9)
    B, D, H, W = shape
    x = torch.randn(*shape, generator=g).to(dtype)
    w = 0.3 * torch.randn(D, 1, 3, 3, generator=g)
    b = 0.1 * torch.randn(D, generator=g) if has_bias else None
    gy = torch.randn(*shape, generator=g).to(dtype)
    xr = x.float().clone().requires_grad_()
    wr = w.clone().requires_grad_()
    br = b.clone().requires_grad_() if has_bias else None
    yr = F.silu(F.conv2d(xr, wr, br, padding=1, groups=D))
    yr.backward(gy.float())
    xd = x.to(DEV).requires_grad_()
    wd = w.to(DEV).requires_grad_()
    bd = b.to(DEV).requires_grad_() if has_bias else None
    y = dwconv3x3_silu_fn(xd, wd, bd, True)
    y.backward(gy.to(DEV))
    tol = _tol(dtype)
    assert y.dtype == dtype
    assert_close(y.float().cpu(), yr.detach(), tol, tol, "y")
    assert_close(xd.grad.float().cpu(), xr.grad, tol, tol * float(xr.grad.abs().max()), "dx")
    assert_close(wd.grad.cpu(), wr.grad, tol, tol * float(wr.grad.abs().max()), "dw")
    if has_bias:
        assert_close(bd.grad.cpu(), br.grad, tol, tol * float(br.grad.abs().max()), "db")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(40, 96, 56, 56), (40, 192, 28, 28), (48, 384, 14, 14), (24, 768, 7, 7),
                                   (11, 16, 56, 56), (9, 8, 28, 28)])       # strip kernels: a ragged last group of 8 samples
def test_dwconv3x3_silu_plane_pipeline(shape):
    """Batches deep enough that one wave / workgroup walks several planes of its channel (the software-pipelined loop
    of dwconv7_kernel, both the shared-plane and the wave-private variant), against plain PyTorch fp32."""
    test_dwconv3x3_silu_matches_torch_fp32(shape, torch.bfloat16, True)


SS2D_SHAPES = [
    # (B, D, H, W, N, dtype)
    (2, 96, 56, 56, 1, torch.float32),      # backbone stage 0 (multi-chunk rows)
    (2, 192, 28, 28, 1, torch.bfloat16),    # stage 1
    (2, 96, 56, 56, 1, torch.bfloat16),     # stage 0 in bf16: the two-waves-per-SIMD kernels (ss2d_l3.hip; 7 chunk rows, tail row of 8 lanes)
    (16, 8, 56, 56, 1, torch.bfloat16),     # batch % 8 == 0: XCD-local sample placement of ss2d_l3.hip (two samples per XCD)
    (8, 24, 28, 28, 1, torch.bfloat16),     # ... at 28 x 28 (four planes per tile, several tile groups per sample)
    (2, 8, 48, 48, 1, torch.bfloat16),      # XFMamba-B @384 stage 1 on ss2d_l3.hip (5 chunk rows, 32-lane tail)
    (8, 16, 24, 24, 1, torch.bfloat16),     # ... stage 2 (2 chunk rows, 8-lane tail, four planes per tile)
    (3, 96, 14, 14, 1, torch.float32),      # stage 2 (4 planes per wavefront)
    (2, 96, 7, 7, 1, torch.bfloat16),       # stage 3
    (2, 32, 7, 7, 16, torch.float32),       # deep fusion block shape (N = 16)
    (1, 16, 12, 9, 4, torch.float32),       # non-square map, odd sizes
    (1, 8, 96, 96, 1, torch.float32),       # XFMamba-B @384 stage 0 plane
    (2, 6, 96, 96, 1, torch.bfloat16),      # ... in bf16: the one-plane-per-tile lean variants (18 chunk rows, sums in registers)
    (1, 5, 3, 5, 2, torch.float32),         # tile of one plane (D not a multiple of 2)
]


@pytest.mark.parametrize("shape", SS2D_SHAPES, ids=[f"B{s[0]}D{s[1]}H{s[2]}W{s[3]}N{s[4]}{str(s[5])[6:]}" for s in SS2D_SHAPES])
def test_fused_ss2d_matches_oracle_chain(shape):
    """xfm_ss2d_fwd/_bwd == cross_merge(selective_scan(cross_scan(.))) of the oracle (reference chain
    models/fusion_vmamba.py:1145-1174), forward and all gradients."""
    from xfmamba_amd.ss2d import ss2d_core_fn, to_route_order
    Bt, D, H, W, N, dt = shape
    L = H * W
    g = torch.Generator().manual_seed(21)
    x = torch.randn(Bt, D, H, W, generator=g).to(dt)
    dts = (0.5 * torch.rand(Bt, 4, D, L, generator=g)).to(dt)          # natural order per route
    Bs = torch.randn(Bt, 4, N, L, generator=g).to(dt)
    Cs = torch.randn(Bt, 4, N, L, generator=g).to(dt)
    A = -0.5 * torch.rand(4 * D, N, generator=g) - 0.05
    Dp = torch.randn(4 * D, generator=g)
    bias = 0.5 * torch.rand(4 * D, generator=g)
    gy = torch.randn(Bt, D, L, generator=g)

    def route(t):   # natural (B,4,C,L) -> what route k sees in its walking order, incl. reversal for k=2,3
        return torch.stack([O.cross_scan_ref(t[:, k].reshape(Bt, -1, H, W))[:, k] for k in range(4)], dim=1)

    leaves = [t.float().clone().requires_grad_() for t in (x, dts, A, Bs, Cs, Dp, bias)]
    xr, dr, Ar, Br, Cr, Dr_, br = leaves
    ys = c_scan.selective_scan_c(O.cross_scan_ref(xr).reshape(Bt, -1, L), route(dr).reshape(Bt, -1, L), Ar,
                                 route(Br), route(Cr), Dr_, br, True, True)
    y_ref = O.cross_merge_ref(ys.view(Bt, 4, D, H, W))
    y_ref.backward(gy)

    hx = x.to(DEV).requires_grad_()
    hd = to_route_order(dts, H, W).to(DEV).requires_grad_()
    hB = to_route_order(Bs, H, W).to(DEV).requires_grad_()
    hC = to_route_order(Cs, H, W).to(DEV).requires_grad_()
    hA, hD, hb = (t.to(DEV).requires_grad_() for t in (A, Dp, bias))
    y = ss2d_core_fn(hx.view(Bt, D, L), hd, hA, hB, hC, hD, hb, H, W)
    y.backward(gy.to(DEV))
    tol = _tol(dt)
    assert_close(y.cpu(), y_ref.detach(), tol, tol * float(y_ref.abs().max()), "y")
    pairs = [("dx", hx.grad, xr.grad), ("ddts", hd.grad, to_route_order(dr.grad, H, W)),
             ("dA", hA.grad, Ar.grad), ("dBs", hB.grad, to_route_order(Br.grad, H, W)),
             ("dCs", hC.grad, to_route_order(Cr.grad, H, W)), ("dD", hD.grad, Dr_.grad), ("dbias", hb.grad, br.grad)]
    for name, got, ref in pairs:
        assert_close(got.float().cpu(), ref, tol, tol * (float(ref.abs().max()) + 1e-6), name)


@pytest.mark.parametrize("shape", [(2, 96, 56, 56), (3, 192, 28, 28), (2, 384, 14, 14), (5, 768, 7, 7), (1, 33, 5, 9),
                                   (2, 256, 24, 20), (1, 512, 12, 12), (2, 1024, 24, 24), (1, 2048, 12, 12),     # XFMamba-B widths
                                   (3, 1536, 7, 7), (1, 520, 9, 5), (32, 768, 7, 7), (21, 384, 14, 14)])                                         # wide rows: 16-wave two-pass kernels
@pytest.mark.parametrize("xdt,ydt", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16),
                                     (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16),
                                     (torch.float32, torch.float16)])      # fp16: a .half() model / default autocast
def test_layernorm2d_matches_torch_fp32(shape, xdt, ydt):
    """LayerNorm2d (reference fusion_vmamba.py:52-57: permute -> F.layer_norm -> permute) vs plain PyTorch fp32."""
    from xfmamba_amd.layernorm2d import layernorm2d_fn
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4)
    B, C, H, W = shape
    x = (torch.randn(*shape, generator=g) * 2 + 0.5).to(xdt)
    w = 1 + 0.2 * torch.randn(C, generator=g)
    b = 0.1 * torch.randn(C, generator=g)
    gy = torch.randn(*shape, generator=g).to(ydt)
    xr = x.float().clone().requires_grad_()
    wr, br = w.clone().requires_grad_(), b.clone().requires_grad_()
    yr = F.layer_norm(xr.permute(0, 2, 3, 1), (C,), wr, br, 1e-5).permute(0, 3, 1, 2)
    yr.backward(gy.float())
    xd = x.to(DEV).requires_grad_()
    wd, bd = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = layernorm2d_fn(xd, wd, bd, 1e-5, ydt)
    y.backward(gy.to(DEV))
    tol = 1e-3 if (xdt == torch.float32 and ydt == torch.float32) else 1e-2
    assert y.dtype == ydt and xd.grad.dtype == xdt
    assert_close(y.float().cpu(), yr.detach(), tol, tol * float(yr.abs().max()), "y")
    assert_close(xd.grad.float().cpu(), xr.grad, tol, tol * float(xr.grad.abs().max()), "dx")
    assert_close(wd.grad.cpu(), wr.grad, tol, tol * float(wr.grad.abs().max()), "dw")
    assert_close(bd.grad.cpu(), br.grad, tol, tol * float(br.grad.abs().max()), "db")


@pytest.mark.parametrize("shape", [(2, 14, 384), (3, 7, 768), (1, 14, 8), (5, 7, 40), (64, 14, 384), (64, 7, 768)])
@pytest.mark.parametrize("with_bias", [True, False])
def test_dwconv3x3_silu_on_token_major_maps_matches_torch_fp32(shape, with_bias):
    """Depthwise 3 x 3 convolution + SiLU (reference fusion_vmamba.py:1198-1201) on TOKEN-MAJOR maps (B, H, W, C) bf16
    (xfm_dwconv3x3_tokens_fwd/_bwd, csrc/dwconv_tok.hip) vs F.conv2d + F.silu in fp32 on the NCHW view: output, dx, dweight,
    dbias; and against the plane-major kernel on the transposed map."""
    import torch.nn.functional as F
    from xfmamba_amd.dwconv import dwconv3x3_silu_fn, dwconv3x3_silu_tokens_fn, dwconv_tokens_supported
    B, HW, C = shape
    g = torch.Generator().manual_seed(B + HW + C)
    x = torch.randn(B, HW, HW, C, generator=g).bfloat16()
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.3
    b = 0.2 * torch.randn(C, generator=g) if with_bias else None
    gy = torch.randn(B, HW, HW, C, generator=g).bfloat16()
    xr, wr = x.float().permute(0, 3, 1, 2).clone().requires_grad_(), w.clone().requires_grad_()
    br = b.clone().requires_grad_() if with_bias else None
    yr = F.silu(F.conv2d(xr, wr, br, padding=1, groups=C))
    yr.backward(gy.float().permute(0, 3, 1, 2))
    xd, wd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    bd = b.to(DEV).requires_grad_() if with_bias else None
    assert dwconv_tokens_supported(xd)
    y = dwconv3x3_silu_tokens_fn(xd, wd, bd)
    y.backward(gy.to(DEV))
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    tol = 1e-2
    assert_close(y.float().cpu(), yr.detach().permute(0, 2, 3, 1), tol, tol * float(yr.abs().max()), "y")
    assert_close(xd.grad.float().cpu(), xr.grad.permute(0, 2, 3, 1), tol, tol * float(xr.grad.abs().max()), "dx")
    assert_close(wd.grad.cpu(), wr.grad, tol, tol * float(wr.grad.abs().max()), "dw")
    if with_bias:
        assert_close(bd.grad.cpu(), br.grad, tol, tol * float(br.grad.abs().max()), "db")
    # the plane-major kernel on the transposed map: the same operator
    xp = x.permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_()
    yp = dwconv3x3_silu_fn(xp, w.to(DEV), None if b is None else b.to(DEV), True)
    assert_close(y.float().cpu(), yp.detach().float().cpu().permute(0, 2, 3, 1), 1e-2, 1e-2 * float(yr.abs().max()), "y vs planes")


# (B, H, W, C, O): the four layers of XFMamba-T at reduced batch, odd sizes (O and 9 C not whole 128-wide tiles, a token count
# that is not a whole 128-token tile or 64-token weight-gradient stage), the smallest map
CONV_S2_SHAPES = [(2, 112, 112, 48, 96), (4, 56, 56, 96, 192), (4, 28, 28, 192, 384), (8, 14, 14, 384, 768),
                  (3, 6, 10, 8, 8), (1, 2, 2, 16, 24), (5, 12, 8, 40, 136), (64, 14, 14, 384, 768), (16, 28, 28, 192, 384)]


@pytest.mark.parametrize("shape", CONV_S2_SHAPES)
def test_conv3x3_stride2_on_token_major_maps_matches_torch_fp32(shape):
    """The trunk's 3 x 3 stride-2 padding-1 convolutions (reference fusion_vmamba.py:1504-1518, 1531-1538) on TOKEN-MAJOR maps
    through xfm_conv3x3s2_tokens_fwd/_bwd_data/_bwd_weight (csrc/conv_tok.hip: neighbourhood rows + the library's MFMA GEMMs)
    vs F.conv2d in fp32 on the NCHW view of the same bf16 operands: output, dx, dweight at 1e-2 of the largest value."""
    import torch.nn.functional as F
    from xfmamba_amd import _lib
    from xfmamba_amd.conv_tokens import conv3x3s2_tokens_fn
    B, H, W, C, O = shape
    g = torch.Generator().manual_seed(B + H + C + O)
    x = torch.randn(B, H, W, C, generator=g).bfloat16()
    w = (torch.randn(O, C, 3, 3, generator=g) * (9 * C) ** -0.5).bfloat16().float()     # (bf16-exact: the kernel reads a bf16 shadow)
    gy = torch.randn(B, H // 2, W // 2, O, generator=g).bfloat16()
    xr, wr = x.float().permute(0, 3, 1, 2).clone().requires_grad_(), w.clone().requires_grad_()
    yr = F.conv2d(xr, wr, None, stride=2, padding=1)
    yr.backward(gy.float().permute(0, 3, 1, 2))
    xd, wd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    assert _lib.lib().xfm_conv3x3s2_tokens_supported(C, O, H, W)
    y = conv3x3s2_tokens_fn(xd, wd)
    y.backward(gy.to(DEV))
    assert y.dtype == torch.bfloat16 and y.shape == (B, H // 2, W // 2, O)
    tol = 1e-2
    assert_close(y.float().cpu(), yr.detach().permute(0, 2, 3, 1), tol, tol * float(yr.abs().max()), "y")
    assert_close(xd.grad.float().cpu(), xr.grad.permute(0, 2, 3, 1), tol, tol * float(xr.grad.abs().max()), "dx")
    assert wd.grad.shape == w.shape
    assert_close(wd.grad.cpu(), wr.grad, tol, tol * float(wr.grad.abs().max()), "dw")
    # the weight gradient straight from the input map (the token x token kernel gathers the window taps itself), where covered
    from xfmamba_amd.conv_tokens import conv3x3s2_wgrad_from_map
    covered = bool(_lib.lib().xfm_conv3x3s2_tokens_bwd_weight_x_supported(B, H, W, C, O))
    assert covered == (shape in [(2, 112, 112, 48, 96), (4, 56, 56, 96, 192), (16, 28, 28, 192, 384)])
    if covered:
        gw = conv3x3s2_wgrad_from_map(gy.to(DEV), x.to(DEV), wd.detach())
        assert gw is not None and gw.shape == w.shape
        assert_close(gw.float().cpu(), wr.grad, tol, tol * float(wr.grad.abs().max()), "dw from the map")


@pytest.mark.parametrize("shape", [(2, 224, 224, 3, 48), (3, 10, 6, 3, 48), (1, 2, 2, 1, 8), (5, 32, 48, 4, 96), (64, 224, 224, 3, 48)])
def test_first_patch_embedding_convolution_on_a_replicated_channel_matches_torch_fp32(shape):
    """The first convolution of the patch embedding (reference fusion_vmamba.py:1504-1518) when its input channels are replicas
    of one channel (net_fusionmamba.py:88-104: x.expand(-1, 3, -1, -1)): xfm_conv3x3s2_gray_fwd / _bwd_weight (csrc/conv_tok.hip)
    vs F.conv2d in fp32 on the expanded image with the bf16-rounded weight: output and every slice of the weight gradient."""
    import torch.nn.functional as F
    from xfmamba_amd import _lib
    from xfmamba_amd.conv_tokens import conv3x3s2_gray_fn
    B, H, W, CI, O = shape
    g = torch.Generator().manual_seed(B + H + O)
    x1 = torch.randn(B, H, W, generator=g).bfloat16()
    w = (torch.randn(O, CI, 3, 3, generator=g) * (9 * CI) ** -0.5).bfloat16().float()
    gy = torch.randn(B, H // 2, W // 2, O, generator=g).bfloat16()
    wr = w.clone().requires_grad_()
    yr = F.conv2d(x1.float().unsqueeze(1).expand(-1, CI, -1, -1), wr, None, stride=2, padding=1)
    yr.backward(gy.float().permute(0, 3, 1, 2))
    assert _lib.lib().xfm_conv3x3s2_gray_supported(O, H, W)
    wd = w.to(DEV).requires_grad_()
    y = conv3x3s2_gray_fn(x1.to(DEV), wd)
    y.backward(gy.to(DEV))
    assert y.dtype == torch.bfloat16 and y.shape == (B, H // 2, W // 2, O)
    tol = 1e-2
    assert_close(y.float().cpu(), yr.detach().permute(0, 2, 3, 1), tol, tol * float(yr.abs().max()), "y")
    assert wd.grad.shape == w.shape
    assert_close(wd.grad.cpu(), wr.grad, tol, tol * float(wr.grad.abs().max()), "dw")


@pytest.mark.parametrize("C", [48, 96, 192, 384, 768, 64, 1024])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["plain", "add", "add_scale"])
def test_add_layernorm_rows_matches_torch_fp32(C, dt, mode):
    """x + drop_path(y) followed by LayerNorm (reference fusion_vmamba.py:1325-1337) on the token-major stream vs
    plain PyTorch fp32: both outputs, both input gradients, dw/db; ragged row count (rows % rows-per-wave != 0)."""
    from xfmamba_amd.rowln import add_layernorm_rows_fn, layernorm_rows_fn
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(C)
    B, H, W = 3, 5, 7
    x = torch.randn(B, H, W, C, generator=g) * 2 + 0.5
    y = torch.randn(B, H, W, C, generator=g).to(dt)
    sc = torch.tensor([0.0, 1.25, 1.25]) if mode == "add_scale" else None
    w = 1 + 0.2 * torch.randn(C, generator=g)
    b = 0.1 * torch.randn(C, generator=g)
    gh = torch.randn(B, H, W, C, generator=g).to(dt)
    gres = torch.randn(B, H, W, C, generator=g)
    xr, yr = x.clone().requires_grad_(), y.float().clone().requires_grad_()
    wr, br = w.clone().requires_grad_(), b.clone().requires_grad_()
    sr = xr if mode == "plain" else xr + (yr if sc is None else yr * sc.view(B, 1, 1, 1))
    hr = F.layer_norm(sr, (C,), wr, br, 1e-5)
    ((hr * gh.float()).sum() + (0 if mode == "plain" else (sr * gres).sum())).backward()
    xd, yd = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
    wd, bd = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    if mode == "plain":
        h = layernorm_rows_fn(xd, wd, bd, 1e-5, dt)
        (h.float() * gh.to(DEV).float()).sum().backward()
    else:
        xn, h = add_layernorm_rows_fn(xd, yd, None if sc is None else sc.to(DEV), wd, bd, 1e-5, dt)
        assert xn.dtype == torch.float32
        assert_close(xn.detach().cpu(), sr.detach(), 1e-6, 1e-6, "x_new")
        ((h.float() * gh.to(DEV).float()).sum() + (xn * gres.to(DEV)).sum()).backward()
    tol = 1e-3 if dt == torch.float32 else 1e-2
    assert h.dtype == dt
    assert_close(h.float().cpu(), hr.detach(), tol, tol * float(hr.abs().max()), "h")
    assert_close(xd.grad.cpu(), xr.grad, tol, tol * float(xr.grad.abs().max()), "dx")
    if mode != "plain":
        assert yd.grad.dtype == dt
        assert_close(yd.grad.float().cpu(), yr.grad, tol, tol * float(yr.grad.abs().max()), "dy")
    assert_close(wd.grad.cpu(), wr.grad, tol, tol * float(wr.grad.abs().max()), "dw")
    assert_close(bd.grad.cpu(), br.grad, tol, tol * float(br.grad.abs().max()), "db")


def test_add_layernorm_rows_many_rows_and_unsupported_width():
    """Grid-stride path (more row groups than workgroups in the backward) and the loud failure for other widths."""
    from xfmamba_amd.rowln import layernorm_rows_fn, rows_supported
    import torch.nn.functional as F
    C = 96
    x = torch.randn(8, 112, 112, C, device=DEV)
    w = (1 + 0.1 * torch.randn(C, device=DEV)).requires_grad_()
    b = torch.zeros(C, device=DEV).requires_grad_()
    xr = x.clone().requires_grad_()
    xd = x.clone().requires_grad_()
    gh = torch.randn_like(x)
    h = layernorm_rows_fn(xd, w, b, 1e-5, torch.float32)
    h.backward(gh)
    dw, db = w.grad.clone(), b.grad.clone()
    w.grad = b.grad = None
    hr = F.layer_norm(xr, (C,), w, b, 1e-5)
    hr.backward(gh)
    assert_close(h.detach().cpu(), hr.detach().cpu(), 1e-4, 1e-4, "h")
    assert_close(xd.grad.cpu(), xr.grad.cpu(), 1e-3, 1e-4, "dx")
    assert_close(dw.cpu(), w.grad.cpu(), 1e-3, 1e-3 * float(w.grad.abs().max()), "dw")
    assert_close(db.cpu(), b.grad.cpu(), 1e-3, 1e-3 * float(b.grad.abs().max()), "db")
    assert not rows_supported(100)
    with pytest.raises(RuntimeError):
        layernorm_rows_fn(torch.randn(2, 3, 100, device=DEV), torch.ones(100, device=DEV), None)


@pytest.mark.parametrize("rows,C", [(37, 384), (3 * 56 * 56, 384), (1000, 768), (64, 3072), (5, 40), (70000, 96)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_bias_gelu_and_colsum_match_torch_fp32(rows, C, dt):
    """fc1 bias + exact GELU (reference Mlp, fusion_vmamba.py:135-153) and the bias-gradient column sums."""
    from xfmamba_amd.mlp_tokens import bias_gelu_fn, colsum_fn
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(rows + C)
    z = (torch.randn(rows, C, generator=g) * 1.5).to(dt)
    b = 0.3 * torch.randn(C, generator=g)
    gy = torch.randn(rows, C, generator=g).to(dt)
    zr, br = z.float().clone().requires_grad_(), b.clone().requires_grad_()
    yr = F.gelu(zr + br)
    yr.backward(gy.float())
    zd, bd = z.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = bias_gelu_fn(zd, bd)
    y.backward(gy.to(DEV))
    tol = 1e-3 if dt == torch.float32 else 1e-2
    assert y.dtype == dt and zd.grad.dtype == dt
    assert_close(y.float().cpu(), yr.detach(), tol, tol * float(yr.abs().max()), "gelu")
    assert_close(zd.grad.float().cpu(), zr.grad, tol, tol * float(zr.grad.abs().max()), "dz")
    assert_close(bd.grad.cpu(), br.grad, tol, tol * float(br.grad.abs().max()) * (1 if dt == torch.float32 else 3), "db")
    cs = colsum_fn(z.to(DEV))
    ref = z.double().sum(0)
    assert_close(cs.cpu(), ref, 1e-4, 1e-4 * float(z.float().abs().sum(0).max()), "colsum")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_mlp_tokens_matches_torch_fp32(dt):
    from xfmamba_amd.mlp_tokens import mlp_tokens_fn
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(11)
    B, H, W, C = 2, 14, 14, 96
    x = torch.randn(B, H, W, C, generator=g)
    w1, b1 = 0.1 * torch.randn(4 * C, C, generator=g), 0.1 * torch.randn(4 * C, generator=g)
    w2, b2 = 0.1 * torch.randn(C, 4 * C, generator=g), 0.1 * torch.randn(C, generator=g)
    gy = torch.randn(B, H, W, C, generator=g)
    ref = [t.clone().requires_grad_() for t in (x, w1, b1, w2, b2)]
    yr = F.linear(F.gelu(F.linear(ref[0], ref[1], ref[2])), ref[3], ref[4])
    yr.backward(gy)
    dev = [t.to(DEV).requires_grad_() for t in (x, w1, b1, w2, b2)]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
        y = mlp_tokens_fn(dev[0].to(dt), *dev[1:])
    y.float().backward(gy.to(DEV))
    tol = 1e-3 if dt == torch.float32 else 1e-2
    assert y.dtype == dt
    assert_close(y.float().cpu(), yr.detach(), tol, tol * float(yr.abs().max()), "y")
    for name, a, r in zip(("dx", "dw1", "db1", "dw2", "db2"), dev, ref):
        assert a.grad.dtype == torch.float32
        assert_close(a.grad.cpu(), r.grad, tol, 2 * tol * float(r.grad.abs().max()), name)


@pytest.mark.parametrize("C,T", [(192, 2 * 28 * 28), (384, 8 * 14 * 14 + 5), (768, 32 * 7 * 7)])
def test_mlp_fused_gelu_products_match_torch_fp32_and_the_unfused_chain(C, T):
    """xfm_tokens_gemm2 (csrc/tokens_gemm.hip): fc1 with z / gelu(z + b1) out of the product's epilogue, fc2's data gradient
    times gelu'(z + b1) out of its own -- reference models/fusion_vmamba.py:135-153 (fc1 -> GELU -> fc2) -- against torch fp32
    at the bf16 bound, and bit for bit against the three-node chain (GEMM, bias + GELU kernel, GEMM) it replaces on the values
    the two share (z, g, dz are rounded to bf16 at the same points)."""
    import torch.nn.functional as F
    from xfmamba_amd import mlp_tokens as M
    g = torch.Generator().manual_seed(C + T)
    x = torch.randn(T, C, generator=g)
    w1, b1 = C ** -0.5 * torch.randn(4 * C, C, generator=g), 0.1 * torch.randn(4 * C, generator=g)
    w2, b2 = (4 * C) ** -0.5 * torch.randn(C, 4 * C, generator=g), 0.1 * torch.randn(C, generator=g)
    gy = torch.randn(T, C, generator=g)
    ref = [t.clone().requires_grad_() for t in (x.bfloat16().float(), w1, b1, w2, b2)]
    yr = F.linear(F.gelu(F.linear(ref[0], ref[1], ref[2])), ref[3], ref[4])
    yr.backward(gy)
    outs = []
    for fused in (True, False):
        old = M._FUSED
        M._FUSED = fused
        try:
            dev = [t.to(DEV).requires_grad_() for t in (x, w1, b1, w2, b2)]
            timer = None
            from xfmamba_amd import _lib
            timer = _lib.KernelTimer()
            _lib.set_timer(timer)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = M.mlp_tokens_fn(dev[0].bfloat16(), *dev[1:])
            y.float().backward(gy.to(DEV))
            _lib.set_timer(None)
            ran = set(timer.summary())
            assert ("mlp_fc1_gelu" in ran and "mlp_fc2_dgrad_gelu" in ran) == fused, ran
            outs.append([y.detach().float().cpu()] + [t.grad.float().cpu() for t in dev])
        finally:
            M._FUSED = old
    names = ("y", "dx", "dw1", "db1", "dw2", "db2")
    for name, a, r in zip(names, outs[0], [yr.detach()] + [t.grad for t in ref]):
        assert_close(a, r, 1e-2, 2e-2 * float(r.abs().max()), name)
    for name, a, b in zip(names, outs[0], outs[1]):                    # the unfused chain rounds at the same points
        assert_close(a, b, 2e-3, 2e-3 * float(b.abs().max()) + 1e-7, name + " (fused vs chain)")


@pytest.mark.parametrize("T,con,out", [(12544 + 37, 384, 1536), (3136, 768, 256), (640, 64, 128), (129, 1536, 384), (3136 + 5, 96, 384), (777, 160, 128)])
@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_tokens_gemm2_tiled_form_every_epilogue_and_weight_layout(T, con, out, wt, epi):
    """xfm_tokens_gemm2 at shapes only its tiled form covers (csrc/tokens_gemm.hip: 128 x 128 tiles, LDS-direct operand ring;
    any con % 64 == 0, out % 128 == 0): plain product + bias, z / gelu(z + b) pair, dz = (x W) gelu'(z + b) -- reference
    models/fusion_vmamba.py:135-153 -- for both weight layouts ((out, con) and (con, out)) against torch fp32 on the same bf16
    operands; token counts that are not multiples of the tile, a single k-stage (con = 64), one n-tile."""
    from xfmamba_amd import _lib
    lib = _lib.lib()
    if not lib.xfm_tokens_gemm2_supported(con, out):
        pytest.skip("tiled form switched off (XFM_GEMM2_FORM)")
    g = torch.Generator().manual_seed(T + con + out + 7 * wt + epi)
    x = torch.randn(T, con, generator=g).bfloat16()
    w = (con ** -0.5 * torch.randn(out, con, generator=g)).bfloat16()
    b = 0.3 * torch.randn(out, generator=g)
    zin = torch.randn(T, out, generator=g).bfloat16()
    acc = x.float() @ w.float().t()
    xd, bd, zd = x.to(DEV), b.to(DEV), zin.to(DEV)
    wd = (w.t().contiguous() if wt else w).to(DEV)
    y = torch.full((T, out), float("nan"), dtype=torch.bfloat16, device=DEV)
    y2 = torch.full((T, out), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.check(lib.xfm_tokens_gemm2(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), y2.data_ptr() if epi == 1 else None,
                                    zd.data_ptr() if epi == 2 else None, T, con, out, wt, epi, _lib.stream_ptr()), "tokens_gemm2")
    torch.cuda.synchronize()
    tol = 1e-2
    if epi == 0:
        r = acc + b
        assert_close(y.float().cpu(), r, tol, tol * float(r.abs().max()), "y")
    elif epi == 1:
        zr = acc.bfloat16().float()                                      # z is rounded before the bias and the GELU see it
        assert_close(y.float().cpu(), acc, tol, tol * float(acc.abs().max()), "z")
        gr = torch.nn.functional.gelu(y.float().cpu() + b)               # (from the z the kernel stored: same rounding point)
        assert_close(y2.float().cpu(), gr, tol, tol * float(gr.abs().max()), "g")
        assert zr.shape == acc.shape
    else:
        zb = (zin.float() + b).requires_grad_()
        torch.nn.functional.gelu(zb).backward(acc.bfloat16().float())    # dg is rounded to bf16 before gelu' multiplies it
        assert_close(y.float().cpu(), zb.grad, tol, tol * float(zb.grad.abs().max()), "dz")


@pytest.mark.parametrize("C,xdt,hdt", [(48, torch.bfloat16, torch.bfloat16), (96, torch.bfloat16, torch.float32),
                                       (192, torch.float32, torch.float32), (768, torch.bfloat16, torch.float32)])
def test_layernorm_rows_with_conv_bias_and_bf16_input(C, xdt, hdt):
    """LayerNorm(conv_out + conv_bias) on tokens (patch-embed / downsample, fusion_vmamba.py:1504-1538): the bias add
    and its gradient live in the norm kernel; the convolution output may arrive in bf16."""
    from xfmamba_amd.rowln import layernorm_rows_fn
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(C + 1)
    x = (torch.randn(4, 9, 11, C, generator=g) * 2).to(xdt)
    pb = torch.randn(C, generator=g)
    w = 1 + 0.2 * torch.randn(C, generator=g)
    b = 0.1 * torch.randn(C, generator=g)
    gh = torch.randn(4, 9, 11, C, generator=g).to(hdt)
    ref = [t.clone().requires_grad_() for t in (x.float(), pb, w, b)]
    hr = F.layer_norm(ref[0] + ref[1], (C,), ref[2], ref[3], 1e-5)
    hr.backward(gh.float())
    dev = [t.to(DEV).requires_grad_() for t in (x, pb, w, b)]
    h = layernorm_rows_fn(dev[0], dev[2], dev[3], 1e-5, hdt, dev[1])
    h.backward(gh.to(DEV))
    tol = 1e-3 if (xdt == torch.float32 and hdt == torch.float32) else 1e-2
    assert h.dtype == hdt and dev[0].grad.dtype == xdt
    assert_close(h.float().cpu(), hr.detach(), tol, tol * float(hr.abs().max()), "h")
    for name, a, r in zip(("dx", "dpre_bias", "dw", "db"), dev, ref):
        assert_close(a.grad.float().cpu(), r.grad, tol, 2 * tol * float(r.grad.abs().max()), name)


def _ss2d_plan_chunks(B, D, H, W, N, dt):
    """n_chunks of xfm_ss2d_plan, 0 when the plan needs no checkpoint buffer."""
    import ctypes
    from xfmamba_amd import _lib
    plan = _lib.ScanPlan()
    _lib.check(_lib.lib().xfm_ss2d_plan(B, D, H, W, N, _lib.dtype_code(dt), ctypes.byref(plan)), "ss2d_plan")
    return plan.n_chunks if plan.n_chunks > 1 else 0


# (the 48 x 48 / 24 x 24 shapes at XFMamba-B's channel counts fill every CU with two workgroups at batch 2: the configuration in
#  which a 16-byte buffer store's data registers were overwritten behind it -- csrc/ss2d_w.hpp, w_st16)
# (56 x 56 and 24 x 24 run their last chunk row one position per lane -- csrc/ss2d_w.hpp, WTail1 --: one sample, an odd batch, the
#  widths of XFMamba-S, a single tile per workgroup)
@pytest.mark.parametrize("shape", [(2, 96, 56, 56, 1), (3, 192, 28, 28, 1), (2, 384, 14, 14, 1), (2, 64, 10, 6, 2),
                                   (2, 256, 48, 48, 1), (2, 1024, 24, 24, 1), (8, 192, 28, 28, 1), (1, 96, 56, 56, 1),
                                   (3, 192, 56, 56, 1), (5, 64, 24, 24, 1), (16, 16, 56, 56, 1)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_ss2d_proj_core_matches_operator_chain(shape, dt):
    """Route split + dt_proj + fused scan as one node (xfm_ss2d_route_split/_merge inside) vs the same maths spelled
    with framework ops around ss2d_core_fn (to_route_order + matmul): output and every gradient."""
    from xfmamba_amd.ss2d import ss2d_core_fn, ss2d_proj_core_fn, to_route_order
    B, D, H, W, N = shape
    L, K = H * W, 4
    R = max(1, D // 16)
    C2 = R + 2 * N
    g = torch.Generator().manual_seed(B * D + H)
    x = torch.randn(B, D, L, generator=g).to(dt)
    xd = (0.5 * torch.randn(B, K * C2, L, generator=g)).to(dt)
    dtw = torch.randn(K, D, R, generator=g) * R ** -0.5
    A = -torch.rand(K * D, N, generator=g) - 0.1
    Dp = torch.randn(K * D, generator=g)
    bias = 0.1 * torch.rand(K * D, generator=g)
    gy = torch.randn(B, D, L, generator=g)
    outs = []
    for fused in (False, True):
        t = [v.to(DEV).requires_grad_() for v in (x, xd, dtw, A, Dp, bias)]
        if fused:
            y = ss2d_proj_core_fn(t[0], t[1], t[2], t[3], t[4], t[5], H, W)
        else:
            r = to_route_order(t[1].view(B, K, C2, L), H, W)
            dts = torch.matmul(t[2].to(dt), r[:, :, :R])
            y = ss2d_core_fn(t[0], dts, t[3], r[:, :, R:R + N].contiguous(), r[:, :, R + N:].contiguous(), t[4], t[5], H, W)
        # the checkpoint buffer the node saved is sized for the kernel family that ran: on the wide maps one state per 512-position
        # chunk row (ss2d_l3.hip: mode 1 here, and mode 2 without fp32 B / C rows), one per lane with them (ss2d_w.hpp: the default
        # bf16 mode-2 call); the plan's chunking on every other shape and dtype
        saved = y.grad_fn.saved_tensors
        chk, b32 = (saved[9], saved[13]) if fused else (saved[7], None)
        rows = 0 if chk is None else chk.shape[3]
        if dt == torch.bfloat16 and N == 1 and H == W and H in (56, 48, 28, 24):
            assert b32 is not None or not fused or H != 56
            assert rows == (L + 511) // 512 * (64 if b32 is not None else 1), (fused, rows)
        else:
            assert b32 is None and rows == _ss2d_plan_chunks(B, D, H, W, N, dt), rows
        y.backward(gy.to(DEV))
        outs.append([y.detach()] + [v.grad for v in t])
    tol = 1e-4 if dt == torch.float32 else 1e-2
    for name, a, b in zip(("y", "dx", "dx_dbl", "ddt_w", "dA", "dD", "dbias"), outs[1], outs[0]):
        assert a.dtype == b.dtype, name
        assert_close(a.float().cpu(), b.float().cpu(), tol, tol * float(b.float().abs().max()) + 1e-7, name)


def test_kernel_timer_brackets_the_wide_map_scan_itself():
    """xfm_prof_main_kernel: the per-kernel timer of bench.py hands its event pair to the library, which records it around the
    wide-map backward scan only; the sum of the workgroups' partial dB / dC rows behind it is a record of its own.  Paths without
    the hook (a short map: no finishing kernel) keep the whole-call bracket, and no pair stays pending."""
    from xfmamba_amd import _lib
    from xfmamba_amd.ss2d import ss2d_proj_core_fn
    g = torch.Generator().manual_seed(5)
    got = {}
    for (B, D, H) in ((8, 96, 56), (2, 64, 10)):
        L, K, N, R = H * H, 4, 1, max(1, D // 16)
        t = [v.to(DEV).requires_grad_() for v in (torch.randn(B, D, L, generator=g).bfloat16(), (0.5 * torch.randn(B, K * (R + 2 * N), L, generator=g)).bfloat16(),
                                                  torch.randn(K, D, R, generator=g) * R ** -0.5, -torch.rand(K * D, N, generator=g) - 0.1,
                                                  torch.randn(K * D, generator=g), 0.1 * torch.rand(K * D, generator=g))]
        timer = _lib.KernelTimer()
        _lib.set_timer(timer)
        try:
            for _ in range(3):
                ss2d_proj_core_fn(*t, H, H).float().sum().backward()
        finally:
            _lib.set_timer(None)
        got[H] = timer.summary()
        assert _lib.lib().xfm_prof_main_kernel(None, None) == 0
    wide, short = got[56], got[10]
    assert "ss2d_bwd_finish" in wide and wide["ss2d_bwd"]["launches"] == wide["ss2d_bwd_finish"]["launches"] == 3
    assert 0 < wide["ss2d_bwd_finish"]["avg_us"] < wide["ss2d_bwd"]["avg_us"]
    assert "ss2d_bwd" in short and "ss2d_bwd_finish" not in short and short["ss2d_bwd"]["avg_us"] > 0


@pytest.mark.parametrize("shape", [(2, 96, 56, 56, 1), (2, 384, 14, 14, 1), (2, 64, 10, 6, 2), (1, 32, 96, 96, 1)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_ss2d_xproj_core_matches_operator_chain(shape, dt):
    """x_proj inside the node (its data gradient accumulated onto the scan's dx by the GEMM) vs x_proj as a framework
    matmul in front of ss2d_proj_core_fn: output and every gradient, incl. x_proj_weight."""
    from xfmamba_amd.ss2d import ss2d_proj_core_fn, ss2d_xproj_core_fn
    B, D, H, W, N = shape
    L, K = H * W, 4
    R = max(1, D // 16)
    C2 = R + 2 * N
    g = torch.Generator().manual_seed(B * D + W)
    x = torch.randn(B, D, L, generator=g).to(dt)
    xw = torch.randn(K, C2, D, generator=g) * D ** -0.5
    dtw = torch.randn(K, D, R, generator=g) * R ** -0.5
    A = -torch.rand(K * D, N, generator=g) - 0.1
    Dp = torch.randn(K * D, generator=g)
    bias = 0.1 * torch.rand(K * D, generator=g)
    gy = torch.randn(B, D, L, generator=g)
    outs = []
    for inside in (False, True):
        t = [v.to(DEV).requires_grad_() for v in (x, xw, dtw, A, Dp, bias)]
        if inside:
            y = ss2d_xproj_core_fn(t[0], t[1], t[2], t[3], t[4], t[5], H, W)
        else:
            xd = torch.matmul(t[1].reshape(K * C2, D).to(dt), t[0])
            y = ss2d_proj_core_fn(t[0], xd, t[2], t[3], t[4], t[5], H, W)
        y.backward(gy.to(DEV))
        outs.append([y.detach()] + [v.grad for v in t])
    tol = 1e-4 if dt == torch.float32 else 1e-2
    for name, a, b in zip(("y", "dx", "dx_proj_w", "ddt_w", "dA", "dD", "dbias"), outs[1], outs[0]):
        assert a.dtype == b.dtype, name
        assert_close(a.float().cpu(), b.float().cpu(), tol, tol * float(b.float().abs().max()) + 1e-7, name)


DTFUSED_SHAPES = [
    # (B, D, H, R): dt_proj INSIDE the wide-map scan kernels (delta_softplus 3, csrc/ss2d_l3.hip) -- built for dt_rank 6 at
    # 56 x 56 and dt_rank 12 at 28 x 28 (XFMamba-T / -S stages 0 / 1); odd ranks exercise the zero padding to Rp
    (2, 96, 56, 6),         # stage 0 of XFMamba-T: 7 chunk rows with an 8-lane tail row, row 5 of the dB / dC sums in LDS
    (16, 8, 56, 6),         # batch % 8 == 0: XCD-local sample placement, several planes per workgroup
    (1, 5, 56, 5),          # rank 5 padded to 6, odd channel count
    (3, 192, 28, 12),       # stage 1: four planes per tile, 2 chunk rows, 34-lane tail
    (8, 24, 28, 12),
    (2, 8, 28, 11),         # rank 11 padded to 12
]


@pytest.mark.parametrize("shape", DTFUSED_SHAPES, ids=[f"B{s[0]}D{s[1]}H{s[2]}R{s[3]}" for s in DTFUSED_SHAPES])
def test_ss2d_with_dt_proj_inside_matches_oracle(shape, monkeypatch):
    """x_proj -> split -> dt_proj -> softplus -> 4-route scan -> merge with the step sizes formed INSIDE the scan kernels
    (reference models/fusion_vmamba.py:1145-1174) against the fp32 CPU oracle chain (cross_scan_ref,
    _proj_dt_B_C, the C scan, cross_merge_ref): y and every gradient; no dt_proj forward kernel may run, no (B,4,D,L) step-size
    tensor may be allocated.  Also against the materialised-step-size path (XFM_SS2D_DT_FUSED=0) of the same node."""
    from xfmamba_amd import _lib, ss2d
    B, D, H, R = shape
    W, N, K = H, 1, 4
    L, C2 = H * W, R + 2
    g = torch.Generator().manual_seed(B * D + R)
    x = torch.randn(B, D, H, W, generator=g).bfloat16()
    xw = (torch.randn(K, C2, D, generator=g) * D ** -0.5).bfloat16().float()        # (the values the bf16 GEMM sees)
    dtw = (torch.randn(K, D, R, generator=g) * R ** -0.5).bfloat16().float()
    A = -torch.rand(K * D, N, generator=g) - 0.1
    Dp = torch.randn(K * D, generator=g)
    bias = torch.rand(K * D, generator=g) * 4 - 4.5               # softplus argument around -2.5: step sizes 0.01 .. 0.5
    gy = torch.randn(B, D, L, generator=g)
    ref = [t.float().clone().requires_grad_() for t in (x, xw, dtw, A, Dp, bias)]
    xs = O.cross_scan_ref(ref[0])
    dts, Bs, Cs = O._proj_dt_B_C(xs, ref[1], ref[2], R, N)
    ys = c_scan.selective_scan_c(xs.reshape(B, -1, L), dts.reshape(B, -1, L), ref[3], Bs.contiguous(), Cs.contiguous(),
                                 ref[4], ref[5], True, True)
    y_ref = O.cross_merge_ref(ys.view(B, K, D, H, W))
    y_ref.backward(gy)
    assert _lib.lib().xfm_ss2d_dtfused_rank(B, D, H, W, N, R, _lib.dtype_code(torch.bfloat16)) == (R + 1) // 2 * 2
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(ss2d, "_DT_FUSED", fused)
        timer = _lib.KernelTimer()
        _lib.set_timer(timer)
        t = [v.to(DEV).requires_grad_() for v in (x.view(B, D, L), xw, dtw, A, Dp, bias)]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = ss2d.ss2d_xproj_core_fn(t[0], t[1], t[2], t[3], t[4], t[5], H, W)
        y.backward(gy.to(DEV))
        _lib.set_timer(None)
        ran = set(timer.summary())
        assert ("dt_proj_fwd" in ran) == (not fused) and ("xr_rows" in ran) == fused, sorted(ran)
        outs[fused] = [y.detach()] + [v.grad for v in t]
    names = ("y", "dx", "dx_proj_w", "ddt_w", "dA", "dD", "dbias")
    refs = [y_ref.detach().view(B, D, L)] + [r.grad for r in ref]
    for name, a, r in zip(names, outs[True], refs):
        r = r.reshape(a.shape)
        assert_close(a.float().cpu(), r, 1e-2, 1e-2 * (float(r.abs().max()) + 1e-6), name)      # BASELINE: 1e-2 for bf16 I/O
    for name, a, b in zip(names, outs[True], outs[False]):
        assert_close(a.float().cpu(), b.float().cpu(), 1e-2, 1e-2 * float(b.float().abs().max()) + 1e-7, name + " vs mode 2")


@pytest.mark.parametrize("shape", [(8, 24, 56, 56), (8, 48, 28, 28), (2, 16, 48, 48), (8, 32, 24, 24)])
def test_ss2d_backward_workspace_entry_equals_the_atomics_entry(shape, monkeypatch):
    """xfm_ss2d_bwd_ws (per-workgroup dB / dC partial rows in a caller workspace + one summing kernel, the default from
    Python) against xfm_ss2d_bwd's flush by fp32 atomics (XFM_L3_ATOMICS=1 makes xfm_ss2d_bwd_ws_bytes return 0) on the
    wide-map kernels: every gradient of the node, incl. the x_proj weight that consumes dB / dC."""
    import ctypes
    from xfmamba_amd import _lib
    from xfmamba_amd.ss2d import ss2d_xproj_core_fn
    B, D, H, W = shape
    L, K, N = H * W, 4, 1
    R = max(1, D // 16)
    g = torch.Generator().manual_seed(D + H)
    x = torch.randn(B, D, L, generator=g).bfloat16()
    xw = torch.randn(K, R + 2 * N, D, generator=g) * D ** -0.5
    dtw = torch.randn(K, D, R, generator=g) * R ** -0.5
    A = -torch.rand(K * D, N, generator=g) - 0.1
    Dp = torch.randn(K * D, generator=g)
    bias = 0.1 * torch.rand(K * D, generator=g)
    gy = torch.randn(B, D, L, generator=g)
    p = _lib.SS2DParams()
    p.batch, p.d_inner, p.H, p.W, p.dstate = B, D, H, W, N
    p.in_dtype, p.out_dtype = _lib.dtype_code(torch.bfloat16), _lib.dtype_code(torch.float32)
    outs = []
    for atomics in (False, True):
        if atomics:
            monkeypatch.setenv("XFM_L3_ATOMICS", "1")
        else:
            monkeypatch.delenv("XFM_L3_ATOMICS", raising=False)
        wsb = _lib.lib().xfm_ss2d_bwd_ws_bytes(ctypes.byref(p))
        assert (wsb == 0) == atomics, (atomics, wsb)
        t = [v.to(DEV).requires_grad_() for v in (x, xw, dtw, A, Dp, bias)]
        y = ss2d_xproj_core_fn(t[0], t[1], t[2], t[3], t[4], t[5], H, W)
        y.backward(gy.to(DEV))
        outs.append([y.detach()] + [v.grad for v in t])
    for name, a, b in zip(("y", "dx", "dx_proj_w", "ddt_w", "dA", "dD", "dbias"), outs[0], outs[1]):
        assert_close(a.float().cpu(), b.float().cpu(), 2e-3, 2e-3 * float(b.float().abs().max()) + 1e-7, name)


@pytest.mark.parametrize("B,D,R,H", [(2, 96, 6, 56), (2, 192, 12, 28), (3, 384, 24, 14), (2, 64, 5, 10), (1, 32, 3, 6)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_dt_proj_kernels_match_torch_fp32(B, D, R, H, with_bias):
    """dt_proj (`einsum("b k r l, k d r -> b k d l")`, fusion_vmamba.py:1154-1156) with the optional bias + softplus
    epilogue (csms6s.py:49-50): the VALU kernel (fp32 and bf16 I/O) and the bf16 MFMA kernel vs plain PyTorch fp32."""
    import ctypes
    import torch.nn.functional as F
    from xfmamba_amd import _lib
    lib = _lib.lib()
    L = H * H
    g = torch.Generator().manual_seed(D + R)
    xr = torch.randn(B, 4, R, L, generator=g)
    w = torch.randn(4, D, R, generator=g) * R ** -0.5
    bias = (torch.rand(4 * D, generator=g) * 4 - 3) if with_bias else None
    st = _lib.stream_ptr()
    for dt in (torch.float32, torch.bfloat16):
        xd = xr.to(dt).to(DEV)
        wq = w.to(dt).float()                                             # the weights the kernel is given
        ref = torch.einsum("bkrl,kdr->bkdl", xd.float().cpu(), wq)
        if with_bias:
            ref = F.softplus(ref + bias.view(1, 4, D, 1))
        out = torch.empty(B, 4, D, L, dtype=dt, device=DEV)
        bd = None if bias is None else bias.to(DEV)
        wd = wq.to(DEV).contiguous()
        _lib.check(lib.xfm_ss2d_dt_proj_fwd(xd.data_ptr(), wd.data_ptr(), _lib.ptr(bd), out.data_ptr(), B, D, R, L,
                                            _lib.dtype_code(dt), st), "dt_proj_fwd")
        tol = 1e-4 if dt == torch.float32 else 1e-2
        assert_close(out.float().cpu(), ref, tol, tol * float(ref.abs().max()), f"VALU {dt}")
        if dt == torch.bfloat16 and lib.xfm_ss2d_dt_proj_mfma_rp(D, R, L):
            out2 = torch.full_like(out, float("nan"))
            wb = w.to(dt).to(DEV).contiguous()
            _lib.check(lib.xfm_ss2d_dt_proj_fwd_mfma(xd.data_ptr(), wb.data_ptr(), _lib.ptr(bd), out2.data_ptr(), B, D, R,
                                                     L, st), "dt_proj_fwd_mfma")
            assert_close(out2.float().cpu(), ref, tol, tol * float(ref.abs().max()), "MFMA bf16")


def test_dt_proj_softplus_epilogue_over_the_whole_range():
    """The softplus of the dt_proj epilogues (csrc/xfm_common.hpp softplus20_16bit; reference models/csms6s.py:49-50:
    F.softplus with threshold 20) for pre-activations from -25 to 25 -- step sizes from 1e-11 up, the linear branch above 20 --
    against torch fp32 at the RELATIVE bf16 bound: the form without a log1p series must keep e^x for tiny step sizes."""
    import torch.nn.functional as F
    from xfmamba_amd import _lib
    lib = _lib.lib()
    B, D, R, H = 1, 96, 6, 56
    L = H * H
    # one rank carries the value, weight 1: raw[d, l] = xr[0, l]; the sweep covers [-25, 25]
    xr = torch.zeros(B, 4, R, L)
    xr[:, :, 0] = torch.linspace(-25.0, 25.0, L)
    w = torch.zeros(4, D, R)
    w[:, :, 0] = 1.0
    bias = torch.zeros(4 * D)
    xd = xr.bfloat16().to(DEV)
    ref = F.softplus(xd.float().cpu()[:, :, 0]).unsqueeze(2).expand(B, 4, D, L)            # (bf16-rounded arguments)
    st = _lib.stream_ptr()
    outs = {}
    out = torch.empty(B, 4, D, L, dtype=torch.bfloat16, device=DEV)
    wd, wb, bd = w.to(DEV).contiguous(), w.bfloat16().to(DEV).contiguous(), bias.to(DEV)
    _lib.check(lib.xfm_ss2d_dt_proj_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, D, R, L,
                                        _lib.dtype_code(torch.bfloat16), st), "dt_proj_fwd")
    outs["VALU"] = out.float().cpu()
    if lib.xfm_ss2d_dt_proj_mfma_rp(D, R, L):
        out2 = torch.full_like(out, float("nan"))
        _lib.check(lib.xfm_ss2d_dt_proj_fwd_mfma(xd.data_ptr(), wb.data_ptr(), bd.data_ptr(), out2.data_ptr(), B, D, R, L, st),
                   "dt_proj_fwd_mfma")
        outs["MFMA"] = out2.float().cpu()
    for name, o in outs.items():
        rel = ((o - ref).abs() / ref).max()
        assert float(rel) < 8e-3, (name, float(rel))                                        # one bf16 ulp = 2^-8 relative
        assert float(o.min()) > 0                                                           # never flushed to zero


@pytest.mark.parametrize("B,D,R,H", [(2, 96, 6, 56), (2, 192, 12, 28), (3, 384, 24, 14), (2, 64, 5, 10),
                                     (1, 1024, 32, 24),       # XFMamba-B stage 2: 66 KB of LDS (opt-in above 64 KB)
                                     # one pass over ddts for both products (a (b, k) slab per workgroup, B * 4 >= 128):
                                     (32, 96, 6, 56), (32, 192, 12, 28), (33, 128, 8, 12), (32, 256, 16, 12),
                                     # XFMamba-S stage 0 (192 channels, rank 6: the two-tile ring with few live rank rows) and
                                     # every store-count bucket of the three-tile ring
                                     (32, 192, 6, 56), (32, 192, 8, 28), (32, 96, 12, 28), (32, 96, 24, 14), (32, 96, 32, 14),
                                     (32, 96, 10, 14)])
def test_dt_proj_backward_mfma_matches_torch_fp32(B, D, R, H):
    """Backward of dt_proj on MFMA (bf16): data gradient W^T.ddts and weight gradient sum_{b,l} ddts.xr^T vs fp32."""
    from xfmamba_amd import _lib
    lib = _lib.lib()
    L = H * H
    g = torch.Generator().manual_seed(D * R)
    ddts = torch.randn(B, 4, D, L, generator=g).to(torch.bfloat16)
    xr = torch.randn(B, 4, R, L, generator=g).to(torch.bfloat16)
    w = (torch.randn(4, D, R, generator=g) * R ** -0.5).to(torch.bfloat16)
    dxr_ref = torch.einsum("kdr,bkdl->bkrl", w.float(), ddts.float())
    dw_ref = torch.einsum("bkdl,bkrl->kdr", ddts.float(), xr.float())
    dd, xd, wd = ddts.to(DEV), xr.to(DEV), w.to(DEV)
    dxr = torch.full((B, 4, R, L), float("nan"), dtype=torch.bfloat16, device=DEV)
    dw = torch.zeros(4, D, R, device=DEV)
    _lib.check(lib.xfm_ss2d_dt_proj_bwd_mfma(dd.data_ptr(), xd.data_ptr(), wd.data_ptr(), dxr.data_ptr(), dw.data_ptr(), B, D,
                                             R, L, _lib.stream_ptr()), "dt_proj_bwd_mfma")
    assert_close(dxr.float().cpu(), dxr_ref, 1e-2, 1e-2 * float(dxr_ref.abs().max()), "dxr")
    assert_close(dw.cpu(), dw_ref, 1e-3, 1e-3 * float(dw_ref.abs().max()), "dw")


def test_kernels_with_counted_waits_under_a_second_process():
    """tools/stress2.py in two processes at once: the merged dt_proj backward at the trunk's stage-0 and stage-1 shapes (and the
    other ring kernels), every result compared with the first.  Memory contention from the other process is what a too-short counted vmcnt wait needs to
    show (round 5: trips 0 and 1 of the three-tile ring did not wait for their own tiles -- 31 of 300 launches wrong)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for op, n in (("dtbwd0", 150), ("dtbwd1", 150), ("dtbwd2", 150),
                  # the other kernels with rings / counted waits / LDS-direct loads, at the trunk's shapes (fewer launches: they are
                  # larger): the wide-map and channel-lane SS2D cores forward + backward, the tiled token GEMM, both token x token
                  # weight-gradient forms
                  # (the wide-map cores 600 times each: the withdrawn register-order flush of round 6 failed 0.1 - 25 % of them)
                  ("l3_56", 600), ("l3_28", 600), ("w_48", 600), ("w_24", 600), ("chan14", 40), ("chan7", 40), ("gemm3", 40),
                  ("wgrad", 40), ("wgradx", 40), ("wgradpp", 300)):
        ps = [subprocess.Popen([sys.executable, os.path.join(root, "tools", "stress2.py"), op, str(n)], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True) for _ in range(2)]
        outs = [p.communicate(timeout=600)[0] for p in ps]
        for p, o in zip(ps, outs):
            assert p.returncode == 0, o[-2000:]
            assert f"{op}: 0 of {n} runs differ" in o, o[-2000:]


@pytest.mark.parametrize("C,xdt,odt", [(48, torch.bfloat16, torch.bfloat16), (48, torch.float32, torch.bfloat16),
                                        (96, torch.float32, torch.float32), (384, torch.bfloat16, torch.bfloat16)])
@pytest.mark.parametrize("with_pre", [True, False])
def test_layernorm_rows_with_gelu_inside_matches_torch_fp32(C, xdt, odt, with_pre):
    """gelu(LayerNorm(x + pre_bias)) -- norm -> GELU of the patch embedding (reference fusion_vmamba.py:1504-1518) -- as one
    kernel each way (xfm_layernorm_rows_gelu_fwd/_bwd) vs F.gelu(F.layer_norm(.)) in fp32: output, dx, dw, db, d pre_bias; and
    against the two-kernel chain it replaces (layernorm_rows_fn + bias_gelu_fn)."""
    import torch.nn.functional as F
    from xfmamba_amd.rowln import layernorm_rows_fn, layernorm_rows_gelu_fn
    from xfmamba_amd.mlp_tokens import bias_gelu_fn
    g = torch.Generator().manual_seed(C + 11)
    B, H, W = 3, 9, 7                                     # 189 rows: not a multiple of the rows a wave holds
    x = (torch.randn(B, H, W, C, generator=g) * 1.5 + 0.3).to(xdt)
    w = 1 + 0.2 * torch.randn(C, generator=g)
    b = 0.3 * torch.randn(C, generator=g)
    pre = 0.5 * torch.randn(C, generator=g) if with_pre else None
    gh = torch.randn(B, H, W, C, generator=g).to(odt)
    ref = [t.clone().requires_grad_() for t in (x.float(), w, b)] + ([pre.clone().requires_grad_()] if with_pre else [])
    yr = F.gelu(F.layer_norm(ref[0] + (ref[3] if with_pre else 0.0), (C,), ref[1], ref[2], 1e-5))
    yr.backward(gh.float())
    dev = [t.to(DEV).requires_grad_() for t in (x, w, b)] + ([pre.to(DEV).requires_grad_()] if with_pre else [])
    y = layernorm_rows_gelu_fn(dev[0], dev[1], dev[2], 1e-5, odt, dev[3] if with_pre else None)
    y.backward(gh.to(DEV))
    tol = 1e-2 if torch.bfloat16 in (xdt, odt) else 1e-4
    assert y.dtype == odt
    assert_close(y.float().cpu(), yr.detach(), tol, tol * float(yr.abs().max()), "y")
    assert_close(dev[0].grad.float().cpu(), ref[0].grad, tol, tol * float(ref[0].grad.abs().max()), "dx")
    assert_close(dev[1].grad.cpu(), ref[1].grad, tol, tol * float(ref[1].grad.abs().max()), "dw")
    assert_close(dev[2].grad.cpu(), ref[2].grad, tol, tol * float(ref[2].grad.abs().max()), "db")
    if with_pre:
        assert_close(dev[3].grad.cpu(), ref[3].grad, tol, tol * float(ref[3].grad.abs().max()), "d pre_bias")
    if odt == torch.bfloat16 and C % 8 == 0:
        y2 = bias_gelu_fn(layernorm_rows_fn(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, odt, None if pre is None else pre.to(DEV)), None)
        assert_close(y.float().cpu(), y2.float().cpu(), 1e-2, 1e-2 * float(yr.abs().max()), "y vs the two-kernel chain")


@pytest.mark.parametrize("C,dt", [(96, torch.float32), (384, torch.bfloat16), (768, torch.bfloat16)])
def test_add_layernorm_rows_with_deferred_linear_bias(C, dt):
    """x + drop_path(y + b2) followed by LayerNorm, with the bias of the linear layer that produced y (Mlp.fc2,
    fusion_vmamba.py:135-153) added inside the kernel: outputs and all gradients incl. d b2 vs plain PyTorch fp32."""
    from xfmamba_amd.rowln import add_layernorm_rows_fn
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(C + 3)
    B, H, W = 4, 6, 5
    x = torch.randn(B, H, W, C, generator=g)
    y = torch.randn(B, H, W, C, generator=g).to(dt)
    yb = 0.3 * torch.randn(C, generator=g)
    sc = torch.tensor([0.0, 1.25, 1.25, 1.25])
    w = 1 + 0.2 * torch.randn(C, generator=g)
    b = 0.1 * torch.randn(C, generator=g)
    gh = torch.randn(B, H, W, C, generator=g).to(dt)
    gres = torch.randn(B, H, W, C, generator=g)
    ref = [t.clone().requires_grad_() for t in (x, y.float(), yb, w, b)]
    sr = ref[0] + (ref[1] + ref[2]) * sc.view(B, 1, 1, 1)
    hr = F.layer_norm(sr, (C,), ref[3], ref[4], 1e-5)
    ((hr * gh.float()).sum() + (sr * gres).sum()).backward()
    dev = [t.to(DEV).requires_grad_() for t in (x, y, yb, w, b)]
    xn, h = add_layernorm_rows_fn(dev[0], dev[1], sc.to(DEV), dev[3], dev[4], 1e-5, dt, dev[2])
    ((h.float() * gh.to(DEV).float()).sum() + (xn * gres.to(DEV)).sum()).backward()
    tol = 1e-3 if dt == torch.float32 else 1e-2
    assert_close(xn.detach().cpu(), sr.detach(), 1e-5, 1e-5, "x_new")
    assert_close(h.float().detach().cpu(), hr.detach(), tol, tol * float(hr.abs().max()), "h")
    for name, a, r in zip(("dx", "dy", "dy_bias", "dw", "db"), dev, ref):
        assert_close(a.grad.float().cpu(), r.grad, tol, 2 * tol * float(r.grad.abs().max()), name)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [1, 16])
def test_rowscan_strided_and_unaligned_operands(dtype, N):
    """7x7 rows (rowscan kernels): operands that are views -- row stride != 49, or a base that is not 16-byte aligned --
    take the element-wise staging path; the results must equal those of the contiguous (vector-staged) call."""
    import xfmamba_amd
    t = _rand_inputs((2, 2, 64, N, 49, dtype), seed=23)
    dev = {k: v.to(DEV) for k, v in t.items()}
    def run(u, delta, Bm, Cm):
        leaves = [x.detach().requires_grad_() for x in (u, delta, Bm, Cm)]
        A, D, bias = (dev[k].detach().requires_grad_() for k in ("A", "D", "delta_bias"))
        y = xfmamba_amd.selective_scan_fn(leaves[0], leaves[1], A, leaves[2], leaves[3], D, bias, True, True)
        y.backward(dev["dout"].to(y.dtype))
        return [y.detach()] + [x.grad for x in leaves] + [A.grad, D.grad, bias.grad]
    ref = run(dev["u"], dev["delta"], dev["B"], dev["C"])
    def wide(x):                                             # row stride 60
        big = torch.zeros(*x.shape[:-1], 60, device=DEV, dtype=x.dtype)
        big[..., 3:52] = x
        return big[..., 3:52]
    def shifted(x):                                          # contiguous rows, base off by 3 elements
        flat = torch.zeros(x.numel() + 3, device=DEV, dtype=x.dtype)
        flat[3:] = x.reshape(-1)
        return flat[3:].view(x.shape)
    for name, f in (("wide", wide), ("shifted", shifted)):
        got = run(f(dev["u"]), f(dev["delta"]), f(dev["B"]), f(dev["C"]))
        for i, (a, b) in enumerate(zip(got, ref)):
            r = 1e-5 if i < 3 else 1e-3                      # y, du, ddelta: same arithmetic; the rest go through atomics
            assert_close(a.float().cpu(), b.float().cpu(), r, r * (float(b.float().abs().max()) + 1e-6), f"{name}[{i}]")


@pytest.mark.gpu
@pytest.mark.parametrize("T,K,N", [(6272, 96, 384), (6272, 384, 96), (4099, 96, 384), (4133, 384, 96), (4096, 96, 96),
                                   (5000, 96, 192)])
@pytest.mark.parametrize("bias", [False, True])
def test_tokens_gemm_linear_matches_torch(T, K, N, bias):
    """Skinny token-major linear layer on MFMA (xfm_tokens_gemm, Mlp.fc1 / fc2 at the 56x56 stage): value, data
    gradient (same kernel, weight staged transposed) and weight / bias gradients against plain PyTorch fp32; row counts
    that are not a multiple of the 32-row tile included."""
    from xfmamba_amd import _lib
    from xfmamba_amd.mlp_tokens import linear_tokens_fn, _skinny_ok
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5)
    b = torch.randn(N, generator=g) if bias else None
    gy = torch.randn(T, N, generator=g).to(torch.bfloat16)
    xr, wr = x.float().requires_grad_(), w.to(torch.bfloat16).float().requires_grad_()
    br = b.clone().requires_grad_() if bias else None
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(gy.float())
    xd, wd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    bd = b.to(DEV).requires_grad_() if bias else None
    assert _skinny_ok(xd, wd.detach().to(torch.bfloat16))      # (the data gradient uses the kernel when (N, K) is built too)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = linear_tokens_fn(xd, wd, bd)
    y.backward(gy.to(DEV))
    assert y.dtype == torch.bfloat16
    assert_close(y.float().cpu(), yr.detach(), 1e-2, 1e-2 * float(yr.abs().max()), "y")
    assert_close(xd.grad.float().cpu(), xr.grad, 1e-2, 1e-2 * float(xr.grad.abs().max()), "dx")
    assert_close(wd.grad.float().cpu(), wr.grad, 1e-2, 1e-2 * float(wr.grad.abs().max()), "dw")
    if bias:
        assert_close(bd.grad.float().cpu(), br.grad, 1e-2, 1e-2 * float(br.grad.abs().max()), "db")


@pytest.mark.gpu
@pytest.mark.parametrize("in_tokens,out_tokens", [(True, False), (False, True)])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("B,L,C", [(5, 1024, 96), (8, 784, 192), (128, 40, 96),      # (128, 40): samples end inside tiles
                                   # the tiled form (per-sample tiles of 128 positions, LDS-direct operand ring): the 14 x 14 stage
                                   # (196 = 128 + 68: a ragged second tile whose last 16-byte chunk straddles the row end), a
                                   # second tile of 4 positions, whole tiles only
                                   (32, 196, 384), (32, 132, 128), (64, 64, 256)])
def test_batched_proj_mfma_layout_changing(in_tokens, out_tokens, bias, B, L, C):
    """in_proj / out_proj of the 56x56 stage through xfm_proj_gemm (tokens -> planes, planes -> tokens; the backward data
    product is the same kernel with the roles swapped and the weight staged transposed) against an fp32 einsum."""
    from xfmamba_amd.proj import batched_proj, _mfma_proj
    g = torch.Generator().manual_seed(8)
    K = M = C
    xp = torch.randn(B, K, L, generator=g).to(torch.bfloat16)
    w = torch.randn(M, K, generator=g) / K ** 0.5
    bb = torch.randn(M, generator=g) if bias else None
    gy = torch.randn(B, M, L, generator=g).to(torch.bfloat16)
    xr, wr = xp.float().requires_grad_(), w.to(torch.bfloat16).float().requires_grad_()
    br = bb.clone().requires_grad_() if bias else None
    yr = torch.einsum("mk,bkl->bml", wr, xr) + (br[None, :, None] if bias else 0)
    yr.backward(gy.float())
    x = (xp.transpose(1, 2).contiguous() if in_tokens else xp.clone()).to(DEV).requires_grad_()
    wd = w.to(DEV).requires_grad_()
    bd = bb.to(DEV).requires_grad_() if bias else None
    assert _mfma_proj(x.detach(), wd.detach().to(torch.bfloat16), None, in_tokens, out_tokens, False) is not None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = batched_proj(x, wd, bd, in_tokens=in_tokens, out_tokens=out_tokens)
    y.backward((gy.transpose(1, 2).contiguous() if out_tokens else gy).to(DEV))
    yc = (y.transpose(1, 2) if out_tokens else y).float().cpu()
    assert_close(yc, yr.detach(), 1e-2, 1e-2 * float(yr.abs().max()), "y")
    dx = (x.grad.transpose(1, 2) if in_tokens else x.grad).float().cpu()
    assert_close(dx, xr.grad, 1e-2, 1e-2 * float(xr.grad.abs().max()), "dx")
    assert_close(wd.grad.float().cpu(), wr.grad, 1e-2, 1e-2 * float(wr.grad.abs().max()), "dw")
    if bias:
        assert_close(bd.grad.float().cpu(), br.grad, 1e-2, 1e-2 * float(br.grad.abs().max()), "db")


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,C", [(64, 49, 1536), (3, 25, 128), (2, 64, 64), (4, 1, 64)])
def test_tokens_to_planes_pooled_matches_permute_and_mean(B, L, C):
    """xfm_pooled_transpose_fwd/_bwd: the tokens -> planes move with the squeeze pooling (avg_pool of ShallowFuse_SS2Dv4,
    reference fusion_vmamba.py:866) -- planes bit-exact, pooled against the fp32 mean, d t against fp32 autograd."""
    from xfmamba_amd.proj import tokens_to_planes_pooled, PooledTokensToPlanes
    g = torch.Generator().manual_seed(B + L)
    t = torch.randn(B, L, C, generator=g).to(torch.bfloat16)
    gp = torch.randn(B, C, L, generator=g).to(torch.bfloat16)
    gm = torch.randn(B, C, generator=g).to(torch.bfloat16)
    tr = t.float().requires_grad_()
    (tr.transpose(1, 2) * gp.float()).sum().backward(retain_graph=True)
    ((tr.mean(1) * gm.float()).sum()).backward()
    td = t.to(DEV).requires_grad_()
    planes, pooled = tokens_to_planes_pooled(td)
    assert isinstance(planes.grad_fn, PooledTokensToPlanes._backward_cls)
    assert torch.equal(planes.cpu(), t.transpose(1, 2).contiguous())
    assert_close(pooled.float().cpu(), t.float().mean(1), 1e-2, 1e-2, "pooled")
    ((planes.float() * gp.to(DEV).float()).sum() + (pooled.float() * gm.to(DEV).float()).sum()).backward()
    assert_close(td.grad.float().cpu(), tr.grad, 1e-2, 1e-2 * float(tr.grad.abs().max()), "dt")


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,L", [(64, 1536, 49), (3, 128, 25), (2, 64, 64), (5, 192, 8)])
def test_gated_planes_to_tokens_matches_multiply_then_permute(B, C, L):
    """xfm_gated_transpose_fwd/_bwd: (y * gate).permute for out_proj (ShallowFuse_SS2Dv4, reference fusion_vmamba.py:870-871):
    the forward bit-exact against the bf16 multiply + transposing copy, d y and d gate against fp32 autograd."""
    from xfmamba_amd.proj import gated_planes_to_tokens, GatedPlanesToTokens
    g = torch.Generator().manual_seed(B * L)
    yy = torch.randn(B, C, L, generator=g).to(torch.bfloat16)
    gate = torch.rand(B, C, generator=g).to(torch.bfloat16)
    gy = torch.randn(B, L, C, generator=g).to(torch.bfloat16)
    yr, gr = yy.float().requires_grad_(), gate.float().requires_grad_()
    (yr * gr.unsqueeze(-1)).transpose(1, 2).backward(gy.float())
    yd, gd = yy.to(DEV).requires_grad_(), gate.to(DEV).requires_grad_()
    out = gated_planes_to_tokens(yd, gd)
    assert isinstance(out.grad_fn, GatedPlanesToTokens._backward_cls)
    assert torch.equal(out.cpu(), (yy * gate.unsqueeze(-1)).transpose(1, 2).contiguous())
    out.backward(gy.to(DEV))
    assert_close(yd.grad.float().cpu(), yr.grad, 1e-2, 1e-2 * float(yr.grad.abs().max()), "dy")
    assert_close(gd.grad.float().cpu(), gr.grad, 1e-2, 1e-2 * float(gr.grad.abs().max()), "dgate")


@pytest.mark.gpu
@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float32])
def test_views_avg_stack_matches_cat_of_views_and_mean(odt):
    """xfm_views_avg_stack_fwd/_bwd: [view 1 | view 2 | (view 1 + view 2) / 2] (Cross_SS2Dv5's three streams) in the GEMM's
    dtype -- exactly cat + mean + cast -- and its gradient."""
    from xfmamba_amd.fusion_vmamba import _ViewsAvgStack
    g = torch.Generator().manual_seed(77)
    n = torch.randn(2 * 6, 7, 7, 64, generator=g)
    gy = torch.randn(3 * 6, 7, 7, 64, generator=g).to(odt)
    nr = n.clone().requires_grad_()
    ref = torch.cat([nr, (nr[:6] + nr[6:]) / 2], dim=0)
    ref.backward(gy.float())
    nd = n.to(DEV).requires_grad_()
    out = _ViewsAvgStack.apply(nd, odt).view(3 * 6, 7, 7, 64)
    assert out.dtype == odt and torch.equal(out.cpu(), ref.detach().to(odt))
    out.backward(gy.to(DEV))
    assert_close(nd.grad.cpu(), nr.grad, 1e-6, 1e-6, "dn")


@pytest.mark.gpu
@pytest.mark.parametrize("B,HW,C,odt", [(32, 7, 768, torch.bfloat16), (5, 7, 128, torch.float32), (3, 5, 64, torch.bfloat16)])
def test_batchnorm_two_views_on_tokens_matches_batchnorm2d(B, HW, C, odt):
    """xfm_bn_tokens_fwd/_bwd (training-mode BatchNorm2d applied to view 1, then view 2, reference fusion_vmamba.py:906-907, on
    the token matrices) against nn.BatchNorm2d on the NCHW maps in fp32: outputs, running statistics after both views, input
    gradient, weight / bias gradients (summed over the views)."""
    from xfmamba_amd.fusion_vmamba import _BatchNormViews, _bn_views_ok
    g = torch.Generator().manual_seed(C + B)
    xt = (torch.randn(2, B, HW, HW, C, generator=g) * 1.7 + 3.0)             # |mean| > std: the shifted sums matter
    gy = torch.randn(2, B, HW, HW, C, generator=g)
    ref = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        ref.weight.copy_(1 + 0.2 * torch.randn(C, generator=g))
        ref.bias.copy_(0.1 * torch.randn(C, generator=g))
        ref.running_mean.copy_(torch.randn(C, generator=g))
        ref.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    dev = torch.nn.BatchNorm2d(C).to(DEV)
    dev.load_state_dict(ref.state_dict())
    ref.train()
    dev.train()
    xr = xt.clone().requires_grad_()
    yr = torch.stack([ref(xr[0].permute(0, 3, 1, 2)), ref(xr[1].permute(0, 3, 1, 2))]).permute(0, 1, 3, 4, 2)
    yr.backward(gy.to(odt).float())
    xd = xt.to(DEV).view(2, B * HW * HW, C).requires_grad_()
    assert _bn_views_ok(dev, xd)
    y = _BatchNormViews.apply(xd, dev.weight, dev.bias, dev.running_mean, dev.running_var, dev.momentum, dev.eps, odt)
    assert y.dtype == odt
    y.backward(gy.to(odt).to(DEV).view(2, B * HW * HW, C))
    tol = 1e-2 if odt == torch.bfloat16 else 1e-4
    assert_close(y.float().cpu().view_as(yr), yr.detach(), tol, tol * float(yr.abs().max()), "y")
    assert_close(dev.running_mean.cpu(), ref.running_mean, 1e-5, 1e-5, "running_mean")
    assert_close(dev.running_var.cpu(), ref.running_var, 1e-5, 1e-5, "running_var")
    assert_close(xd.grad.cpu().view_as(xr.grad), xr.grad, 1e-4, 1e-4 * float(xr.grad.abs().max()), "dx")
    assert_close(dev.weight.grad.cpu(), ref.weight.grad, 1e-4, 1e-4 * float(ref.weight.grad.abs().max()), "dweight")
    assert_close(dev.bias.grad.cpu(), ref.bias.grad, 1e-4, 1e-4 * float(ref.bias.grad.abs().max()), "dbias")


@pytest.mark.gpu
@pytest.mark.parametrize("B,R,C", [(5, 49, 768), (3, 64, 128), (2, 25, 64), (96, 49, 1536), (1, 1, 64)])
def test_transpose_short_is_the_exact_permutation_both_ways(B, R, C):
    """xfm_transpose_short ((B, R, C) tokens <-> (B, C, R) planes, R <= 64): bit-exact against permute + contiguous, both
    directions, and through autograd (the gradient of one move is the other)."""
    from xfmamba_amd.proj import planes_to_tokens, tokens_to_planes, _transpose_short_ok
    g = torch.Generator().manual_seed(B * 1000 + R)
    t = torch.randn(B, R, C, generator=g).to(torch.bfloat16).to(DEV)
    assert _transpose_short_ok(t, R, C)
    p = tokens_to_planes(t)
    assert p.shape == (B, C, R) and p.is_contiguous()
    assert torch.equal(p, t.transpose(1, 2).contiguous())
    assert torch.equal(planes_to_tokens(p), t)
    tr = t.clone().requires_grad_()
    gy = torch.randn(B, C, R, generator=g).to(torch.bfloat16).to(DEV)
    tokens_to_planes(tr).backward(gy)
    assert torch.equal(tr.grad, gy.transpose(1, 2).contiguous())
    # accumulating form: planes += tokens^T, fp32 add, one rounding
    from xfmamba_amd import _lib
    acc0 = torch.randn(B, C, R, generator=g).to(torch.bfloat16).to(DEV)
    acc = acc0.clone()
    _lib.check(_lib.lib().xfm_transpose_short_add_bf16(t.data_ptr(), acc.data_ptr(), B, R, C, _lib.stream_ptr()), "add")
    assert torch.equal(acc, (acc0.float() + t.transpose(1, 2).float()).to(torch.bfloat16))
    # a shape the kernel does not take goes through the framework's copy
    u = torch.randn(2, 70, 64, generator=g).to(torch.bfloat16).to(DEV)
    assert not _transpose_short_ok(u, 70, 64)
    assert torch.equal(tokens_to_planes(u), u.transpose(1, 2).contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("in_tokens,out_tokens", [(True, False), (False, True)])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("B,L,K,M", [(64, 49, 768, 768), (32, 49, 1536, 768), (8, 25, 128, 192)])
def test_batched_proj_short_maps_one_gemm_plus_transpose(in_tokens, out_tokens, bias, B, L, K, M):
    """Layout-changing projections on 7 x 7 maps (trunk stage 3 in_proj / out_proj, the deep block's out_proj): one GEMM over
    all token rows + xfm_transpose_short, against an fp32 einsum -- value, data, weight and bias gradients."""
    from xfmamba_amd.proj import batched_proj
    g = torch.Generator().manual_seed(L * K)
    xp = torch.randn(B, K, L, generator=g).to(torch.bfloat16)
    w = torch.randn(M, K, generator=g) / K ** 0.5
    bb = torch.randn(M, generator=g) if bias else None
    gy = torch.randn(B, M, L, generator=g).to(torch.bfloat16)
    xr, wr = xp.float().requires_grad_(), w.to(torch.bfloat16).float().requires_grad_()
    br = bb.clone().requires_grad_() if bias else None
    yr = torch.einsum("mk,bkl->bml", wr, xr) + (br[None, :, None] if bias else 0)
    yr.backward(gy.float())
    x = (xp.transpose(1, 2).contiguous() if in_tokens else xp.clone()).to(DEV).requires_grad_()
    wd = w.to(DEV).requires_grad_()
    bd = bb.to(DEV).requires_grad_() if bias else None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = batched_proj(x, wd, bd, in_tokens=in_tokens, out_tokens=out_tokens)
    assert y.shape == ((B, L, M) if out_tokens else (B, M, L)) and y.is_contiguous()
    y.backward((gy.transpose(1, 2).contiguous() if out_tokens else gy).to(DEV))
    yc = (y.transpose(1, 2) if out_tokens else y).float().cpu()
    assert_close(yc, yr.detach(), 1e-2, 1e-2 * float(yr.abs().max()), "y")
    dx = (x.grad.transpose(1, 2) if in_tokens else x.grad).float().cpu()
    assert_close(dx, xr.grad, 1e-2, 1e-2 * float(xr.grad.abs().max()), "dx")
    assert_close(wd.grad.float().cpu(), wr.grad, 1e-2, 1e-2 * float(wr.grad.abs().max()), "dw")
    if bias:
        assert_close(bd.grad.float().cpu(), br.grad, 1e-2, 1e-2 * float(br.grad.abs().max()), "db")


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,D,XC", [(32, 196, 384, 128), (24, 196, 384, 128), (32, 132, 256, 128)])
def test_tiled_xproj_forward_and_accumulating_backward(B, L, D, XC):
    """x_proj of a channel-lane SS2D block at 14 x 14 on the tiled form: planes -> tokens (D -> XC) through xfm_proj_gemm,
    and its data gradient dx += Wx^T . d x_dbl^T (tokens -> planes, XC -> D) through xfm_proj_gemm_accumulate, against
    fp32 matmuls; the accumulation adds in fp32 and rounds once, so it is compared with (dx0 + product) rounded to bf16."""
    from xfmamba_amd import _lib
    from xfmamba_amd.proj import _mfma_proj
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, D, L, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(XC, D, generator=g) / D ** 0.5).to(torch.bfloat16).to(DEV)
    y = _mfma_proj(x, w, None, False, True, False)
    assert y is not None and y.shape == (B, L, XC)
    yr = torch.einsum("cd,bdl->blc", w.float(), x.float())
    assert_close(y.float().cpu(), yr.cpu(), 1e-2, 1e-2 * float(yr.abs().max()), "x_dbl")
    dy = torch.randn(B, L, XC, generator=g).to(torch.bfloat16).to(DEV)
    dx0 = torch.randn(B, D, L, generator=g).to(torch.bfloat16).to(DEV)
    dx = dx0.clone()
    lib = _lib.lib()
    assert lib.xfm_proj_gemm_supported(XC, D, L)
    _lib.check(lib.xfm_proj_gemm_accumulate(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, L, XC, D, 1, _lib.stream_ptr()),
               "proj_gemm_accumulate")
    ref = dx0.float() + torch.einsum("cd,blc->bdl", w.float(), dy.float())
    assert_close(dx.float().cpu(), ref.cpu(), 1e-2, 1e-2 * float(ref.abs().max()), "dx")
    # shapes outside the tiled form are refused, not computed some other way
    assert lib.xfm_proj_gemm_accumulate(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, L, 96, 96, 1, _lib.stream_ptr()) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,D,O", [(4, 3136, 96, 32), (128, 40, 96, 32), (6, 784, 192, 56), (64, 784, 192, 56), (136, 40, 192, 56)])
def test_planes_gemm_xproj_forward_and_accumulating_backward(B, L, D, O):
    """x_proj on the natural map at the 56x56 stage (planes -> planes, 96 -> 32) and at the 28x28 stage (192 -> 4 x 14 = 56 rows:
    padded to MFMA tiles inside the kernel) and its backward data product dx += W^T . d x_dbl (accumulate) through
    xfm_planes_gemm, against fp32 matmuls."""
    from xfmamba_amd.proj import mfma_planes
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, D, L, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(O, D, generator=g) / D ** 0.5).to(torch.bfloat16).to(DEV)
    y = mfma_planes(x, w, O)
    assert y is not None and y.shape == (B, O, L)
    ref = torch.einsum("mk,bkl->bml", w.float(), x.float())
    assert_close(y.float().cpu(), ref.cpu(), 1e-2, 1e-2 * float(ref.abs().max()), "x_dbl")
    dxd = torch.randn(B, O, L, generator=g).to(torch.bfloat16).to(DEV)
    dx0 = torch.randn(B, D, L, generator=g).to(torch.bfloat16).to(DEV)
    dx = dx0.clone()
    assert mfma_planes(dxd, w, D, transposed=True, accumulate_into=dx) is dx
    ref = dx0.float() + torch.einsum("mk,bml->bkl", w.float(), dxd.float())
    assert_close(dx.float().cpu(), ref.cpu(), 1e-2, 1e-2 * float(ref.abs().max()), "dx")


# ---------------------------------------------------------------------------------------------
# token-contracting weight-gradient kernel (csrc/wgrad_gemm.hip)
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("Bt,L,M,N", [(4, 196, 384, 1536), (3, 784, 192, 192), (2, 3136, 96, 384), (5, 49, 768, 128),
                                      (2, 196, 128, 384), (1, 36, 24, 40),
                                      (3, 25, 48, 200),                                 # ragged plane rows, odd length
                                      (1, 4096, 384, 96), (1, 2112, 136, 72)])       # one long token run: the LDS-direct kernel
@pytest.mark.parametrize("a_planes,b_planes", [(False, False), (False, True), (True, False), (True, True)])
def test_wgrad_mfma_matches_torch_fp32(Bt, L, M, N, a_planes, b_planes):
    """dW = sum_{b,l} A[b,l,:]^T B[b,l,:] for every operand-layout pair against the fp32 einsum of the same bf16 operands;
    fp32 accumulation: tolerance 2e-3 of the largest entry (summation order)."""
    from xfmamba_amd.proj import wgrad_mfma
    g = torch.Generator().manual_seed(Bt * L + M + N)
    A = torch.randn(Bt, L, M, generator=g).bfloat16()
    Bm = torch.randn(Bt, L, N, generator=g).bfloat16()
    ref = torch.einsum("blm,bln->mn", A.float(), Bm.float())
    a = (A.transpose(1, 2).contiguous() if a_planes else A).to(DEV)
    b = (Bm.transpose(1, 2).contiguous() if b_planes else Bm).to(DEV)
    dw = wgrad_mfma(a, a_planes, b, b_planes)
    assert dw is not None and dw.dtype == torch.float32
    assert_close(dw.cpu(), ref, 2e-3, 2e-3 * float(ref.abs().max()), "dw")
    # accumulation into a caller buffer, strided samples (a slice of a wider batch)
    wide = torch.randn(Bt, 2, *a.shape[1:], generator=g).bfloat16().to(DEV)
    wide[:, 1] = a
    acc = torch.full((M, N), 1.5, dtype=torch.float32, device=DEV)
    out = wgrad_mfma(wide[:, 1], a_planes, b, b_planes, out=acc)
    if out is not None:                                   # (sample stride must keep the vector alignment)
        assert_close((acc - 1.5).cpu(), ref, 2e-3, 2e-3 * float(ref.abs().max()), "dw (accumulated, strided)")


@pytest.mark.gpu
@pytest.mark.parametrize("ydt,odt", [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32),
                                     (torch.float32, torch.float32), (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("mode", ["full", "noscale", "nobias"])
def test_residual_settle_matches_torch_fp32(ydt, odt, mode):
    """xfm_residual_settle_fwd/_bwd: out = x + scale[b] * (y + y_bias) in the consumer's dtype (the end-of-stage residual add
    of VSSBlock._forward, reference fusion_vmamba.py:1325-1337, feeding the downsample convolution) vs plain PyTorch fp32:
    output, dx, dy, d y_bias; ragged vector count (rows * C / 8 not a multiple of the block size)."""
    from xfmamba_amd.rowln import residual_settle_fn
    g = torch.Generator().manual_seed(9)
    B, H, W, C = 3, 5, 7, 96
    x = torch.randn(B, H, W, C, generator=g)
    y = torch.randn(B, H, W, C, generator=g).to(ydt)
    sc = None if mode == "noscale" else torch.tensor([0.0, 1.25, 1.25])
    yb = None if mode == "nobias" else torch.randn(C, generator=g)
    gy = torch.randn(B, H, W, C, generator=g).to(odt)
    xr, yr = x.clone().requires_grad_(), y.float().clone().requires_grad_()
    ybr = None if yb is None else yb.clone().requires_grad_()
    ref = yr if ybr is None else yr + ybr
    ref = xr + (ref if sc is None else ref * sc.view(B, 1, 1, 1))
    ref.backward(gy.float())
    xd, yd = x.to(DEV).requires_grad_(), y.to(DEV).requires_grad_()
    ybd = None if yb is None else yb.to(DEV).requires_grad_()
    out = residual_settle_fn(xd, yd, None if sc is None else sc.to(DEV), ybd, odt)
    assert out.dtype == odt
    out.backward(gy.to(DEV))
    tol = 1e-6 if (ydt == torch.float32 and odt == torch.float32) else 1e-2
    assert_close(out.float().cpu(), ref.detach(), tol, tol * float(ref.abs().max()), "out")
    assert_close(xd.grad.cpu(), xr.grad, tol, tol * float(xr.grad.abs().max()), "dx")
    assert yd.grad.dtype == ydt
    assert_close(yd.grad.float().cpu(), yr.grad, tol, tol * float(yr.grad.abs().max()) + 1e-7, "dy")
    if yb is not None:
        assert_close(ybd.grad.cpu(), ybr.grad, tol, tol * float(ybr.grad.abs().max()) + 1e-6, "dyb")


@pytest.mark.gpu
def test_partial_sums_multi_folds_many_jobs_in_one_launch():
    """xfm_partial_sums_multi at the C ABI: jobs with 1, 2 and 3 parts, widths that are not multiples of the 64-column
    block, block counts around the 16 / 32 row-slot strides, a null output pointer -- against a plain sum."""
    from xfmamba_amd import _lib
    g = torch.Generator().manual_seed(17)
    specs = [(1, 96, 7), (2, 100, 16), (3, 72, 33), (3, 1536, 130), (1, 8, 1), (2, 64, 48)]       # (parts, C, nblk)
    parts, outs, refs, rows, blocks = [], [], [], [], []
    for ji, (np_, C, nblk) in enumerate(specs):
        p = torch.randn(nblk, np_, C, generator=g).to(DEV)
        o = [torch.full((C,), 7.0, device=DEV) for _ in range(np_)]
        skip = ji == 2                                                       # job 2: second output not wanted
        ptrs = [0 if (skip and k == 1) else o[k].data_ptr() for k in range(np_)] + [0] * (3 - np_)
        rows += [p.data_ptr()] + ptrs + [nblk | (C << 32), np_]
        blocks += [ji | (cb << 16) for cb in range((np_ * C + 63) // 64)]
        parts.append(p); outs.append(o); refs.append(p.double().sum(0).float().cpu())
    jobs_d = torch.tensor(rows, dtype=torch.int64).to(DEV)
    blocks_d = torch.tensor(blocks, dtype=torch.int32).to(DEV)
    _lib.check(_lib.lib().xfm_partial_sums_multi(jobs_d.data_ptr(), blocks_d.data_ptr(), len(blocks), _lib.stream_ptr()),
               "partial_sums_multi")
    torch.cuda.synchronize()
    for ji, (np_, C, nblk) in enumerate(specs):
        for k in range(np_):
            if ji == 2 and k == 1:
                assert float((outs[ji][k] - 7.0).abs().max()) == 0.0      # untouched
                continue
            assert_close(outs[ji][k].cpu(), refs[ji][k], 1e-5, 1e-5 * float(refs[ji][k].abs().max()) + 1e-6, f"job {ji} part {k}")
