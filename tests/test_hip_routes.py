"""GPU checks of the route configurations: ``xfm_cross_scan_flex`` / ``xfm_cross_merge_flex`` against the restatement of
``triton_cross_scan_flex`` (tests/test_cross_routes.py) and the G6 goldens, and SS2Dv2 ``v051d_noz`` / ``v052d_noz`` against
the reference (G6) and the CPU oracle chain with the routes swapped."""
import pytest
import torch

import xfmamba_amd
from oracle import xfm_oracle as O
from tests.helpers import assert_close, bf16_operand_scan, load_npz
from tests.test_cross_routes import (CONFIG_IDS, CONFIGS, G6_SHAPES, config_tag, ref_merge, ref_scan, torch_slip,
                                     x_shape)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 3, 5, 7), (1, 4, 12, 12), (2, 7, 14, 9), (3, 40, 7, 7), (2, 96, 56, 56), (1, 5, 96, 96), (2, 130, 9, 11)]
FP16_CONFIGS = [c for c in CONFIGS if c[3] == 2 or c[2]]


def _y_shape(B, C, H, W, out_cf):
    return (B, 4, C, H, W) if out_cf else (B, H, W, 4, C)


def _dot(a, b):
    return float((a.double().cpu() * b.double().cpu()).sum())


# relative bound of one rounding of an fp32 value to the dtype (merges sum in fp32 and round once)
ROUND = {torch.float32: 1e-6, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _check_config(cfg, dtype, shape, seed=0):
    in_cf, out_cf, obo, scans = cfg
    B, C, H, W = shape
    f = (B, C, H, W, in_cf, out_cf, obo, scans)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*x_shape(B, C, H, W, in_cf, obo), generator=g).to(dtype)
    yin = torch.randn(*_y_shape(B, C, H, W, out_cf), generator=g).to(dtype)
    # scan: bit-exact, and its backward is the adjoint
    xd = x.to(DEV).requires_grad_()
    ys = xfmamba_amd.cross_scan_fn(xd, in_cf, out_cf, obo, scans)
    assert ys.dtype == dtype and ys.is_contiguous()
    assert ys.shape == ((B, 4, C, H * W) if out_cf else (B, H * W, 4, C))
    assert torch.equal(ys.detach().cpu(), ref_scan(x, *f)), "scan"
    gy = torch.randn(*ys.shape, generator=g).to(dtype)
    ys.backward(gy.to(DEV))
    assert xd.grad.shape == x.shape
    # <scan(x), g> = <x, merge(g)> in fp64; a 16-bit merge adds one rounding per element
    adj = 1e-5 if dtype == torch.float32 else ROUND[dtype]
    lhs, rhs = _dot(ys.detach(), gy), _dot(x, xd.grad)
    assert abs(lhs - rhs) <= adj * max(1.0, _dot(ys.detach().abs(), gy.abs())), ("scan adjoint", lhs, rhs)
    # merge: the fp32 sum, rounded once to the output dtype; its backward is the adjoint
    yd = yin.to(DEV).requires_grad_()
    m = xfmamba_amd.cross_merge_fn(yd, in_cf, out_cf, obo, scans)
    ref = ref_merge(yin.float(), *f)
    assert m.dtype == dtype and m.shape == ref.shape and m.is_contiguous()
    err = (m.detach().float().cpu() - ref).abs()
    assert bool((err <= ROUND[dtype] * ref.abs() + 1e-6).all()), ("merge", float(err.max()))
    gm = torch.randn(*m.shape, generator=g).to(dtype)
    m.backward(gm.to(DEV))
    assert torch.equal(yd.grad.cpu(), ref_scan(gm, *f).reshape(yin.shape)), "merge backward = scan"
    lhs, rhs = _dot(m.detach(), gm), _dot(yin, yd.grad)
    assert abs(lhs - rhs) <= adj * max(1.0, _dot(m.detach().abs(), gm.abs())), ("merge adjoint", lhs, rhs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_flex_routes_match_the_restatement(cfg, dtype):
    for i, shape in enumerate(SHAPES):
        _check_config(cfg, dtype, shape, seed=i)


@pytest.mark.parametrize("cfg", FP16_CONFIGS, ids=[CONFIG_IDS[CONFIGS.index(c)] for c in FP16_CONFIGS])
def test_flex_routes_fp16(cfg):
    for i, shape in enumerate(SHAPES[:4] + SHAPES[6:]):
        _check_config(cfg, torch.float16, shape, seed=i)


def test_flex_routes_unaligned_views_and_mixed_merge_dtypes():
    """Vector widths fall back when a base pointer is not 16-byte aligned; the C entry's fp32 -> bf16 merge."""
    from xfmamba_amd import _lib
    B, C, H, W = 2, 16, 8, 8
    base = torch.randn(B * H * W * C + 1, device=DEV).bfloat16()
    x = base[1:].view(B, H, W, C)                              # 2-byte aligned
    y = xfmamba_amd.cross_scan_fn(x, False, False, False, 2)
    assert torch.equal(y.cpu(), ref_scan(x.cpu(), B, C, H, W, False, False, False, 2))
    y32 = torch.randn(B, 4, C, H * W, device=DEV)
    out = torch.empty(B, C, H * W, device=DEV, dtype=torch.bfloat16)
    _lib.check(_lib.lib().xfm_cross_merge_flex(y32.data_ptr(), out.data_ptr(), B, C, H, W, 0, 0, 0, 1, _lib.XFM_F32,
                                               _lib.XFM_BF16, _lib.stream_ptr()), "merge")
    assert torch.equal(out.cpu(), ref_merge(y32.cpu(), B, C, H, W, True, True, False, 1).bfloat16())
    for bad in ((2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 3), (0, 0, 0, -1)):
        assert _lib.lib().xfm_cross_scan_flex(y32.data_ptr(), out.data_ptr(), B, C, H, W, *bad, _lib.XFM_F32,
                                              _lib.stream_ptr()) == -1, bad


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_flex_routes_match_the_g6_golden(cfg):
    z = load_npz("g6_routes.npz")
    in_cf, out_cf, obo, scans = cfg
    for name, (B, C, H, W) in G6_SHAPES.items():
        if torch_slip(*cfg):
            continue
        a = {k: torch.from_numpy(z[f"{name}/{config_tag(*cfg)}/{k}"]) for k in ("x", "scan", "gscan", "dx", "yin", "merge",
                                                                                   "gmerge", "dyin")}
        xd = a["x"].to(DEV).requires_grad_()
        ys = xfmamba_amd.cross_scan_fn(xd, in_cf, out_cf, obo, scans)
        assert torch.equal(ys.detach().cpu(), a["scan"].reshape(ys.shape)), "scan"
        ys.backward(a["gscan"].reshape(ys.shape).to(DEV))
        assert_close(xd.grad.cpu(), a["dx"], 1e-6, 1e-6, "dx")
        yd = a["yin"].to(DEV).requires_grad_()
        m = xfmamba_amd.cross_merge_fn(yd, in_cf, out_cf, obo, scans)
        assert_close(m.detach().cpu(), a["merge"].reshape(m.shape), 1e-6, 1e-6, "merge")
        m.backward(a["gmerge"].reshape(m.shape).to(DEV))
        assert torch.equal(yd.grad.cpu(), a["dyin"]), "dyin"


def test_default_configuration_still_runs_the_existing_kernels():
    from xfmamba_amd import _lib
    x = torch.randn(2, 8, 6, 5, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    try:
        ys = xfmamba_amd.cross_scan_fn(x)
        ys.backward(torch.ones_like(ys))
        m = xfmamba_amd.cross_merge_fn(ys.detach().view(2, 4, 8, 6, 5))
        ran = set(timer.summary())
    finally:
        _lib.set_timer(None)
    assert ran == {"cross_scan", "cross_merge"}, sorted(ran)
    assert torch.equal(ys.detach().cpu(), O.cross_scan_ref(x.detach().cpu()))
    assert m.shape == (2, 8, 30)


# ---- SS2Dv2 v051d / v052d -----------------------------------------------------------------------------------------
def _build(ft, tag):
    from xfmamba_amd import fusion_vmamba as fv
    return fv.SS2Dv2(d_model=16, d_state=1, ssm_ratio=1.0 if tag == "a" else 2.0, dt_rank="auto", conv_bias=False,
                     forward_type=ft, channel_first=True)


FUSED = {"ss2d_fwd", "ss2d_bwd", "ss2dc_fwd", "ss2dc_bwd", "ss2dc16_fwd", "ss2dc16_bwd", "cross_scan", "cross_merge"}


@pytest.mark.parametrize("mode", ["unfused", "fused"])
@pytest.mark.parametrize("ft", ["v051d_noz", "v052d_noz"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_ss2dv2_route_types_match_the_g6_golden(ft, tag, mode):
    from xfmamba_amd import _lib, fusion_vmamba as fv
    z = load_npz("g6_routes.npz")
    key = f"{ft}/{tag}"
    old = fv.SS2D_MODE
    fv.SS2D_MODE = mode
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    try:
        m = _build(ft, tag)
        pre = f"{key}/sd/"
        m.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}, strict=True)
        m = m.to(DEV).eval()
        x = torch.from_numpy(z[f"{key}/in0"]).to(DEV).requires_grad_()
        out = m(x)
        ref = torch.from_numpy(z[f"{key}/out0"])
        assert_close(out.detach().cpu(), ref, 1e-3, 1e-3 * float(ref.abs().max()), "out0")
        out.backward(torch.from_numpy(z[f"{key}/gout0"]).to(DEV))
        ref = torch.from_numpy(z[f"{key}/din0"])
        assert_close(x.grad.cpu(), ref, 1e-3, 1e-3 * float(ref.abs().max()), "din0")
        pre = f"{key}/grad/"
        params = dict(m.named_parameters())
        for k in z.files:
            if k.startswith(pre):
                ref = torch.from_numpy(z[k])
                assert_close(params[k[len(pre):]].grad.cpu(), ref, 1e-3, 1e-3 * float(ref.abs().max()) + 1e-7, k)
        for k, p in params.items():
            assert (p.grad is not None) == ((pre + k) in z.files), k
        ran = set(timer.summary())
    finally:
        _lib.set_timer(None)
        fv.SS2D_MODE = old
    assert {"cross_scan_flex", "cross_merge_flex", "selective_scan_fwd", "selective_scan_bwd"} <= ran, sorted(ran)
    assert not (FUSED & ran), sorted(ran)


def _bf(t):
    return t.bfloat16().float()


@pytest.mark.parametrize("scans", [1, 2])
def test_ss2d_route_core_at_a_production_shape_matches_the_oracle(scans):
    """d_inner 192 (d_model 96), 56 x 56, batch 8, bf16 autocast: the core SS2Dv2 runs for v051d / v052d against the CPU
    oracle chain with the routes swapped (restated maps -> x_proj -> bf16 x_dbl -> dt_proj -> C scan -> merge), samples 0, 7."""
    from xfmamba_amd import _lib
    from xfmamba_amd.fusion_vmamba import _ss2d_core
    Bt, D, H, W, R, N = 8, 192, 56, 56, 6, 1
    L = H * W
    g = torch.Generator().manual_seed(40 + scans)
    x = _bf(torch.randn(Bt, D, H, W, generator=g))
    xw = _bf(torch.randn(4, R + 2 * N, D, generator=g) * D ** -0.5)
    dtw = _bf(torch.randn(4, D, R, generator=g) * R ** -0.5)
    A_logs = torch.log(torch.rand(4 * D, N, generator=g) + 0.1)
    Dp = torch.randn(4 * D, generator=g)
    dt0 = torch.exp(torch.rand(4 * D, generator=g) * 4.6 - 6.9)
    bias = (dt0 + torch.log(-torch.expm1(-dt0))).view(4, D)
    gy = _bf(torch.randn(Bt, D, L, generator=g))
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    try:
        t = [v.to(DEV).requires_grad_() for v in (x.bfloat16(), xw, dtw, A_logs, Dp, bias)]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y, _ = _ss2d_core(t[0], t[1], t[2], t[3], t[4], t[5], scans=scans)
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
        ran = set(timer.summary())
    finally:
        _lib.set_timer(None)
    assert {"cross_scan_flex", "cross_merge_flex", "selective_scan_fwd"} <= ran and not (FUSED & ran), sorted(ran)
    pick = torch.tensor([0, Bt - 1])
    f = (len(pick), D, H, W, True, True, False, scans)
    o = [v.clone().requires_grad_() for v in (x[pick], xw, dtw, A_logs, Dp, bias)]
    xs = ref_scan(o[0], *f)                                                          # (2, 4, D, L)
    x_dbl = torch.einsum("bkdl,kcd->bkcl", xs, o[1])
    x_dbl = x_dbl + (_bf(x_dbl) - x_dbl).detach()
    dts = torch.einsum("bkrl,kdr->bkdl", x_dbl[:, :, :R], o[2])
    ys = bf16_operand_scan(xs.reshape(len(pick), -1, L), dts.reshape(len(pick), -1, L), -o[3].exp(),
                           x_dbl[:, :, R:R + N].contiguous(), x_dbl[:, :, R + N:].contiguous(), o[4], o[5].reshape(-1),
                           True, True)
    y_ref = ref_merge(ys.view(len(pick), 4, D, L), *f)
    y_ref.backward(gy[pick])
    tol = 1e-2
    assert_close(y.detach().float().cpu()[pick], y_ref.detach(), tol, tol * float(y_ref.abs().max()), "y")
    assert_close(t[0].grad.float().cpu()[pick], o[0].grad, tol, tol * float(o[0].grad.abs().max()), "dx")


def test_backbone_with_bidirectional_routes_trains_on_the_gpu():
    from xfmamba_amd import _lib
    from xfmamba_amd.fusion_vmamba import Backbone_VSSM
    torch.manual_seed(0)
    bb = Backbone_VSSM(depths=[1, 1, 1, 1], dims=16, drop_path_rate=0.1, forward_type="v052d_noz", in_chans=3).to(DEV)
    bb.train()
    x = torch.randn(2, 3, 64, 64, device=DEV)
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs = bb(x)
        loss = sum(o.float().square().mean() for o in outs)
        loss.backward()
        ran = set(timer.summary())
    finally:
        _lib.set_timer(None)
    assert torch.isfinite(loss)
    assert {"cross_scan_flex", "cross_merge_flex"} <= ran and not (FUSED & ran), sorted(ran)
    grads = [p.grad for p in bb.parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    xw = [m.x_proj_weight.grad for m in bb.modules() if hasattr(m, "scans")]
    assert len(xw) == 4 and all(float(g.abs().max()) > 0 for g in xw)
