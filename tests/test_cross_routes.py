"""CPU checks of the route configurations of ``cross_scan_fn`` / ``cross_merge_fn`` and the ``v051d`` / ``v052d`` SS2Dv2
forward types: a restatement of the index maps of ``triton_cross_scan_flex`` (models/csm_triton.py:279-400) against the G6
golden vectors recorded from the reference's torch path, the refusal of CPU tensors, and the modules' parameter layout."""
import itertools

import pytest
import torch

import xfmamba_amd
from tests.helpers import load_npz

CONFIGS = list(itertools.product((True, False), (True, False), (False, True), (0, 1, 2)))
CONFIG_IDS = [f"icf{int(a)}-ocf{int(b)}-obo{int(c)}-s{d}" for a, b, c, d in CONFIGS]
G6_SHAPES = {"a": (2, 3, 5, 7), "b": (1, 4, 6, 9)}


def config_tag(in_cf, out_cf, obo, scans):
    return f"{int(in_cf)}{int(out_cf)}{int(obo)}{scans}"


# ---- restatement of the Triton index maps -------------------------------------------------------------------------
def route_positions(H, W, scans):
    """(4, L) long: route k's position q_k(p) for the map position p = h*W + w."""
    h, w = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    L = H * W
    p, t = (h * W + w).reshape(-1), (w * H + h).reshape(-1)
    if scans == 0:
        return torch.stack([p, t, L - 1 - p, L - 1 - t])
    if scans == 1:
        return torch.stack([p, p, p, p])
    return torch.stack([p, p, L - 1 - p, L - 1 - p])


def x_shape(B, C, H, W, in_cf, obo):
    if obo:
        return (B, 4, C, H, W) if in_cf else (B, H, W, 4, C)
    return (B, C, H, W) if in_cf else (B, H, W, C)


def ref_scan(x, B, C, H, W, in_cf, out_cf, obo, scans):
    """y_k[q_k(p)] = x[p] (one_by_one: x_k[p]) -> (B, 4, C, L) | (B, L, 4, C)."""
    L = H * W
    if obo:
        xk = x.reshape(B, 4, C, L) if in_cf else x.reshape(B, L, 4, C).permute(0, 2, 3, 1)
    else:
        xc = x.reshape(B, C, L) if in_cf else x.reshape(B, L, C).transpose(1, 2)
        xk = xc[:, None].expand(B, 4, C, L)
    q = route_positions(H, W, scans)
    y = x.new_empty((B, 4, C, L))
    for k in range(4):
        y[:, k][..., q[k]] = xk[:, k]
    return y if out_cf else y.permute(0, 3, 1, 2).contiguous()


def ref_merge(y, B, C, H, W, in_cf, out_cf, obo, scans):
    """x[p] = y_0[q_0(p)] + y_1[q_1(p)] + y_2[q_2(p)] + y_3[q_3(p)] in y's dtype (one_by_one: x_k[p] = y_k[q_k(p)])
    -> (B, C, L) | (B, L, C) | (B, 4, C, L) | (B, L, 4, C)."""
    L = H * W
    yk = y.reshape(B, 4, C, L) if out_cf else y.reshape(B, L, 4, C).permute(0, 2, 3, 1)
    q = route_positions(H, W, scans)
    v = torch.stack([yk[:, k][..., q[k]] for k in range(4)], dim=1)
    if obo:
        return v.contiguous() if in_cf else v.permute(0, 3, 1, 2).contiguous()
    x = ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]
    return x if in_cf else x.transpose(1, 2).contiguous()


def torch_slip(in_cf, out_cf, obo, scans):
    """Where the reference's torch one_by_one scan differs from its Triton kernel, the contract (csm_triton.py:99, 119-124):
    the golden does not record these configurations."""
    return obo and (((not in_cf) and scans == 2) or (in_cf and not out_cf and scans == 1))


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_restatement_reproduces_the_g6_golden(cfg):
    z = load_npz("g6_routes.npz")
    in_cf, out_cf, obo, scans = cfg
    tag = config_tag(*cfg)
    for name, (B, C, H, W) in G6_SHAPES.items():
        if torch_slip(in_cf, out_cf, obo, scans):
            assert f"{name}/{tag}/scan" not in z.files
            continue
        a = {k: torch.from_numpy(z[f"{name}/{tag}/{k}"])
             for k in ("x", "scan", "gscan", "dx", "yin", "merge", "gmerge", "dyin")}
        f = (B, C, H, W, in_cf, out_cf, obo, scans)
        # pure data movement: bit-exact
        assert torch.equal(ref_scan(a["x"], *f), a["scan"].reshape(ref_scan(a["x"], *f).shape))
        assert torch.equal(ref_scan(a["gmerge"], *f).reshape(a["dyin"].shape), a["dyin"])
        # sums of up to four fp32 terms: the reference's summation order differs by at most a rounding
        for got, ref in ((ref_merge(a["yin"], *f), a["merge"]), (ref_merge(a["gscan"], *f), a["dx"])):
            got = got.reshape(ref.shape)
            torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)
            if obo:
                assert torch.equal(got, ref)


def test_g6_golden_covers_every_configuration_the_torch_path_computes():
    z = load_npz("g6_routes.npz")
    for name in G6_SHAPES:
        for cfg in CONFIGS:
            assert (f"{name}/{config_tag(*cfg)}/scan" in z.files) == (not torch_slip(*cfg)), cfg


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_cpu_tensors_are_refused_in_every_configuration(cfg):
    in_cf, out_cf, obo, scans = cfg
    B, C, H, W = 1, 2, 3, 3
    x = torch.randn(*x_shape(B, C, H, W, in_cf, obo))
    y = torch.randn(*((B, 4, C, H, W) if out_cf else (B, H, W, 4, C)))
    hot = in_cf and out_cf and not obo and scans == 0
    for fn, t in ((xfmamba_amd.cross_scan_fn, x), (xfmamba_amd.cross_merge_fn, y)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(t, in_cf, out_cf, obo, scans)
        if not hot:
            with pytest.raises(NotImplementedError, match="no CPU path"):
                fn(t, in_cf, out_cf, obo, scans)
        with pytest.raises(NotImplementedError):
            fn(t, in_cf, out_cf, obo, scans, force_torch=True)


@pytest.mark.parametrize("scans", [-1, 3])
def test_route_modes_outside_the_built_ones_raise(scans):
    for fn in (xfmamba_amd.cross_scan_fn, xfmamba_amd.cross_merge_fn):
        with pytest.raises(NotImplementedError, match="scans"):
            fn(torch.randn(1, 4, 2, 3, 3), scans=scans)


@pytest.mark.parametrize("ft,scans", [("v051d", 1), ("v051d_noz", 1), ("v052d", 2), ("v052d_noz", 2),
                                      ("v052d_nozact", 2)])
def test_ss2dv2_route_types_build_with_the_reference_parameters(ft, scans):
    from xfmamba_amd.fusion_vmamba import SS2Dv2
    z = load_npz("g6_routes.npz")
    kw = dict(d_model=16, d_state=1, ssm_ratio=1.0, dt_rank="auto", conv_bias=False, channel_first=True)
    torch.manual_seed(0)
    m = SS2Dv2(forward_type=ft, **kw)
    assert m.scans == scans
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    if ft.endswith("_noz"):
        pre = f"{ft}/a/sd/"
        ref = {k[len(pre):]: tuple(z[k].shape) for k in z.files if k.startswith(pre)}
    else:                    # the same parameters as the cross2d type with the same suffix (pinned by the G4 goldens)
        ref = {k: tuple(v.shape) for k, v in SS2Dv2(forward_type="v05" + ft[5:], **kw).state_dict().items()}
    assert sd == ref


def test_backbone_builds_with_a_route_forward_type():
    from xfmamba_amd.fusion_vmamba import Backbone_VSSM, SS2Dv2
    bb = Backbone_VSSM(depths=[1, 1, 1, 1], dims=16, drop_path_rate=0.0, forward_type="v052d_noz")
    ops = [m for m in bb.modules() if isinstance(m, SS2Dv2)]
    assert len(ops) == 4 and all(m.scans == 2 and m.disable_z for m in ops)
