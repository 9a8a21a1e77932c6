"""BASELINE configs[2] (XFMamba-S, 2 x 224^2, batch 32 per GPU) and configs[3] (XFMamba-B hidden_dim 1024, 2 x 384^2, batch 16
per GPU) at their REAL batch sizes.  The launch plans of the SS2D kernels depend on the batch (tile groups per workgroup and
the partial-row workspace of the wide-map kernels, the XCD-local sample maps at batch % 8 == 0, the tile counts of the fused
scans), so the golden fixtures' batch 1 / 2 leave the production plans unchecked.

Part 1: every SS2D core of the two models, at its exact production shape (read off the constructed models), through the entry
the model calls under bf16 autocast, forward and backward, against the CPU oracle chain -- per-sample outputs on every sample,
batch-summed gradients against the oracle summed over ALL samples (fp64 accumulation).  Which kernel family ran is asserted
too, and the XCD sample map is isolated by a run without it in a child process.
Part 2: both whole models at the bench batch under bf16 autocast, eval forward and training backward, against the fp32 oracle
with the oracle's own bf16 run as the yardstick (the rule of the XFMamba-T bench-batch tests in test_hip_model.py)."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from oracle import c_scan
from oracle import xfm_oracle as O
from tests.helpers import MODEL_CFGS, _model_with_synth_weights, assert_close, bf16_operand_scan, load_json

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# per-GPU batch of BASELINE configs[2] / [3]
BENCH = {"small": (MODEL_CFGS["small"], 32), "base384": (MODEL_CFGS["base384"], 16)}
NODE_IDS = [f"{cfg}-{node}" for cfg in BENCH for node in ("s0", "s1", "s2", "s3", "shallow", "deep")]


@functools.lru_cache(maxsize=None)
def _node_table(cfg):
    """{node: (kind, Bt, D, HW, R, N)} read off the constructed model: (d_inner, dt_rank, d_state) of the first SS2D block of
    every stage and of both fusion blocks; the map size from the image size; Bt = 2 x batch on the trunk (the two views run
    as one batch), 2 x batch (two single-route views) in the shallow block, 3 x batch (three streams) in the deep block."""
    from xfmamba_amd.net_fusionmamba import TwoViewXFMambaTop
    (_, ty, kw, size, _), batch = BENCH[cfg]
    m = TwoViewXFMambaTop(in_channels=1, outputs=2, type=ty, **kw)
    out = {}
    for i, layer in enumerate(m.mamba_feature_extrac.layers):
        op = layer.blocks[0].op
        _, D, R = op.dt_projs_weight.shape
        HW = size // 4 >> i
        out[f"s{i}"] = ("chan" if HW <= 14 else "wide", 2 * batch, D, HW, R, op.A_logs.shape[1])
    HW = size // 32
    sh = m.shallow_mamba_fusion.shallowfuseSS2D
    out["shallow"] = ("swap", 2 * batch, sh.dt_projs_weight.shape[1], HW, sh.dt_projs_weight.shape[2], sh.A_logs.shape[1])
    dp = m.fusemamba.blocks[0].self_attention
    out["deep"] = ("deep", 3 * batch, dp.dt_projs_weight.shape[1], HW, dp.dt_projs_weight.shape[2], dp.A_logs.shape[1])
    return out


def test_node_table_matches_the_model_shapes():
    """The table the node tests run is the one of the state shapes (XFMamba-B@384: d_inner / R 256 / 8 at 96 x 96 ...
    2048 / 64 at 12 x 12; XFMamba-S stage 0: 192 / 6 at 56 x 56)."""
    t = _node_table("base384")
    assert [t[f"s{i}"][2:5] for i in range(4)] == [(256, 96, 8), (512, 48, 16), (1024, 24, 32), (2048, 12, 64)]
    assert t["shallow"] == ("swap", 32, 2048, 12, 64, 16) and t["deep"] == ("deep", 48, 2048, 12, 64, 16)
    s = _node_table("small")
    assert s["s0"] == ("wide", 64, 192, 56, 6, 1) and s["s3"] == ("chan", 64, 1536, 7, 48, 1)
    assert s["shallow"][:2] == ("swap", 64) and s["deep"][:2] == ("deep", 96)


def _bf(t):
    return t.bfloat16().float()


def _node_inputs(kind, Bt, D, HW, R, N, seed):
    """Operands in the model regime (same construction as test_hip_chan.py::_inputs): x and the weights bf16-representable,
    step sizes softplus^-1 of 1e-3 .. 1e-1 plus a few in the linear branch of softplus; d_state 16 with the model's
    A = -(1 .. 16).  The swap node's x is route-major [route 0 | route 1] (2 x B, D, L)."""
    g = torch.Generator().manual_seed(seed)
    K = 2 if kind == "swap" else 4
    L, C2 = HW * HW, R + 2 * N
    x = _bf(torch.randn(Bt, D, L, generator=g))
    xw = _bf(torch.randn(K, C2, D, generator=g) * D ** -0.5)
    dtw = _bf(torch.randn(K, D, R, generator=g) * R ** -0.5)
    if N == 1:
        A = -torch.rand(K * D, N, generator=g) - 0.1
    else:
        A = -(torch.arange(1, N + 1, dtype=torch.float32).repeat(K * D, 1)) * (1 + 0.05 * torch.randn(K * D, N, generator=g))
    Dp = torch.randn(K * D, generator=g)
    dt0 = torch.exp(torch.rand(K * D, generator=g) * 4.6 - 6.9)
    bias = dt0 + torch.log(-torch.expm1(-dt0))
    bias[::97] = 21.0
    gy = _bf(torch.randn(Bt, D, L, generator=g))
    return x, xw, dtw, A, Dp, bias, gy


def _oracle_chunk(kind, x, xw, dtw, A, Dp, bias, gy, HW, N, c_mod=0, c_off=0):
    """CPU oracle chain on a few samples: cross_scan (or the swap block's two routes) -> x_proj -> bf16 rounding of x_dbl (the
    kernels' rounding point) -> dt_proj -> C scan -> cross_merge; -> [y, dx, dx_proj_w, ddt_w, dA, dD, dbias].  For the swap
    node ``x`` / ``gy`` are (B, 2, D, L) per sample."""
    R = dtw.shape[2]
    t = [v.clone().requires_grad_() for v in (x, xw, dtw, A, Dp, bias)]
    if kind == "swap":
        xs = t[0]
    else:
        B, D, L = x.shape
        xs = O.cross_scan_ref(t[0].view(B, D, HW, HW))
    B, K, D, L = xs.shape
    x_dbl = torch.einsum("bkdl,kcd->bkcl", xs, t[1])
    x_dbl = x_dbl + (_bf(x_dbl) - x_dbl).detach()
    dts = torch.einsum("bkrl,kdr->bkdl", x_dbl[:, :, :R], t[2])
    Bs, Cs = x_dbl[:, :, R:R + N].contiguous(), x_dbl[:, :, R + N:].contiguous()
    if c_mod > 0:                                   # deep fusion block: every stream reads through the fused stream's C
        Cs = Cs[c_off + torch.arange(B) % c_mod].contiguous()
    ys = c_scan.selective_scan_c(xs.reshape(B, -1, L), dts.reshape(B, -1, L), t[3], Bs, Cs, t[4], t[5], True, True)
    y = ys.view(B, K, D, L) if kind == "swap" else O.cross_merge_ref(ys.view(B, K, D, HW, HW))
    y.backward(gy)
    return [y.detach()] + [v.grad for v in t]


def _oracle_full(kind, Bt, HW, N, x, xw, dtw, A, Dp, bias, gy):
    """The oracle over ALL Bt samples in chunks: per-sample outputs concatenated, the batch-summed gradients accumulated in
    fp64 (a dropped or doubled workgroup partial sum anywhere in the batch shows)."""
    D, L = x.shape[1], HW * HW
    per = max(1, (1 << 25) // (4 * D * L * N))                       # ~32 M scan elements per chunk
    y, dx = torch.empty(Bt, D, L), torch.empty(Bt, D, L)
    sums = [torch.zeros(v.shape, dtype=torch.float64) for v in (xw, dtw, A, Dp, bias)]
    if kind == "deep":                                               # chunks of whole stream triples [view 1 | view 2 | fused]
        B = Bt // 3
        for j0 in range(0, B, per):
            j = torch.arange(j0, min(B, j0 + per))
            idx = torch.cat([j, B + j, 2 * B + j])
            r = _oracle_chunk(kind, x[idx], xw, dtw, A, Dp, bias, gy[idx], HW, N, len(j), 2 * len(j))
            y[idx], dx[idx] = r[0].view(len(idx), D, L), r[1]
            for s, g in zip(sums, r[2:]):
                s += g.double()
    elif kind == "swap":                                             # oracle sample b = routes (b, B + b) of the node
        B = Bt // 2
        xr, gr = x.view(2, B, D, L).transpose(0, 1), gy.view(2, B, D, L).transpose(0, 1)
        yv, dxv = y.view(2, B, D, L).transpose(0, 1), dx.view(2, B, D, L).transpose(0, 1)
        for b0 in range(0, B, per):
            b = slice(b0, min(B, b0 + per))
            r = _oracle_chunk(kind, xr[b].contiguous(), xw, dtw, A, Dp, bias, gr[b].contiguous(), HW, N)
            yv[b], dxv[b] = r[0], r[1]
            for s, g in zip(sums, r[2:]):
                s += g.double()
    else:
        for b0 in range(0, Bt, per):
            b = slice(b0, min(Bt, b0 + per))
            r = _oracle_chunk(kind, x[b], xw, dtw, A, Dp, bias, gy[b], HW, N)
            y[b], dx[b] = r[0].view(-1, D, L), r[1]
            for s, g in zip(sums, r[2:]):
                s += g.double()
    return [y, dx] + sums


def _run_node(cfg, node):
    """The node at its production shape through the entry the model calls, bf16 autocast, forward + backward.
    -> (inputs, [y, dx, dx_proj_w, ddt_w, dA, dD, dbias] on the CPU, kernel families that ran, workspace sizes asked for)."""
    from xfmamba_amd import _lib
    from xfmamba_amd.csms6s import selective_scan_fn
    from xfmamba_amd.ss2d import ss2d_xproj_core_fn
    from xfmamba_amd.ss2d_chan import chan_supported, ss2d_chan_fn, ss2d_chan_swap_fn, ytokens_supported
    kind, Bt, D, HW, R, N = _node_table(cfg)[node]
    L = HW * HW
    ins = _node_inputs(kind, Bt, D, HW, R, N, seed=Bt * D + HW + R)
    x, xw, dtw, A, Dp, bias, gy = ins
    lib = _lib.lib()
    orig, ws_seen = lib.xfm_ss2d_bwd_ws_bytes, []

    def ws_spy(p):
        n = orig(p)
        ws_seen.append(int(n))
        return n
    lib.xfm_ss2d_bwd_ws_bytes = ws_spy                # (the ctypes handle's attribute: what ss2d.py calls)
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    try:
        t = [v.to(DEV).requires_grad_() for v in (x.bfloat16(), xw, dtw, A, Dp, bias)]
        g = gy.to(DEV)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if kind == "wide":
                y = ss2d_xproj_core_fn(t[0], t[1], t[2], t[3], t[4], t[5], HW, HW)
            elif kind == "chan":
                assert chan_supported(t[0], HW, HW, N, 4, D, R), (cfg, node)
                tok = ytokens_supported(HW, HW, N)            # the trunk's short-map blocks take y token-major (fusion_vmamba.py)
                y = ss2d_chan_fn(t[0], t[1], t[2], t[3], t[4], t[5], HW, HW, y_tokens=tok)
                if tok:
                    y = y.transpose(1, 2)
            elif kind == "swap" and chan_supported(t[0], HW, HW, N, 1, D, R):
                y = ss2d_chan_swap_fn(t[0], t[1], t[2], t[3], t[4], t[5], HW, HW)
            elif kind == "swap":
                # maps the swap kernel does not cover (XFMamba-B@384: 12 x 12, d_state 16): the operator chain of
                # ShallowFuse_SS2Dv4.forward_stacked -- x_proj and dt_proj GEMMs, the 2-route scan on (B, 2, D, L)
                B = Bt // 2
                xs = t[0].view(2, B, D, L).transpose(0, 1)
                x_dbl = torch.matmul(t[1].to(xs.dtype), xs)
                dts, Bs, Cs = torch.split(x_dbl, [R, N, N], dim=2)
                dts = torch.matmul(t[2].to(xs.dtype), dts)
                ys = selective_scan_fn(xs.reshape(B, -1, L), dts.reshape(B, -1, L), t[3], Bs.contiguous(), Cs.contiguous(),
                                       t[4], t[5], True, True, None)
                y = ys.view(B, 2, D, L).transpose(0, 1).reshape(Bt, D, L)
            else:
                assert chan_supported(t[0], HW, HW, N, 4, D, R), (cfg, node)
                y = ss2d_chan_fn(t[0], t[1], t[2], t[3], t[4], t[5], HW, HW, Bt // 3, 2 * Bt // 3)
        y.backward(g)
        torch.cuda.synchronize()
        got = [y.detach().float().cpu().reshape(Bt, D, L)] + [v.grad.float().cpu() for v in t]
        ran = set(timer.summary())
    finally:
        _lib.set_timer(None)
        lib.xfm_ss2d_bwd_ws_bytes = orig
    return ins, got, ran, ws_seen


def _swap_kernel_covers(cfg):
    """Whether the channel-lane swap kernel serves the model's shallow fusion block (it is built for 7 x 7 maps)."""
    from xfmamba_amd import _lib
    _, _, D, HW, R, N = _node_table(cfg)["shallow"]
    return bool(_lib.lib().xfm_ss2dc_supported(HW, HW, N, 1, D, R))


def _check_plan(cfg, node, ran, ws_seen):
    """Which kernel family served the node at its production shape.  A later change that moves a production shape onto
    another path must show here (and be re-validated by this file) instead of passing unnoticed."""
    from xfmamba_amd import _lib, ss2d
    kind, Bt, D, HW, R, N = _node_table(cfg)[node]
    L, lib = HW * HW, _lib.lib()
    bf16 = _lib.dtype_code(torch.bfloat16)
    if kind == "wide":
        assert {"ss2d_fwd", "ss2d_bwd"} <= ran and not any(n.startswith("ss2dc") for n in ran), sorted(ran)
        assert len(ws_seen) == 1, ws_seen
        if HW in (56, 48, 28, 24):
            # the wide-map kernels (csrc/ss2d_l3.hip) with several tile groups per sample: the partial-row workspace and
            # ss2d_l3_parts_kernel carry the dB / dC sums (no atomics); the workspace holds whole groups of partial rows
            row = Bt * 4 * 2 * L * 4
            assert ws_seen[0] > 0 and ws_seen[0] % row == 0 and ws_seen[0] // row > 1, (ws_seen, row)
            if ss2d._DT_FUSED and lib.xfm_ss2d_dtfused_rank(Bt, D, HW, HW, N, R, bf16) > 0:
                assert "xr_rows" in ran and "dt_proj_fwd" not in ran, sorted(ran)      # dt_proj inside the scan (mode 3)
            else:
                # dt_proj kernel + the fourth-generation kernels (ss2d_w.hpp) reading fp32 B / C rows
                assert "dt_proj_fwd" in ran and lib.xfm_ss2d_bc_f32(Bt, D, HW, HW, N, bf16) == 1, sorted(ran)
        else:
            # 96 x 96 (XFMamba-B@384 stage 0): the one-plane-per-tile lean kernels, dB / dC by atomics, no workspace
            assert HW == 96 and ws_seen == [0] and "dt_proj_fwd" in ran, (ws_seen, sorted(ran))
    elif kind == "swap" and not _swap_kernel_covers(cfg):
        # XFMamba-B@384's shallow block (12 x 12, d_state 16): the operator chain with the plain scan kernels
        assert {"selective_scan_fwd", "selective_scan_bwd"} <= ran and not any(n.startswith("ss2dc") for n in ran), sorted(ran)
    else:
        fam = {"chan": "ss2dc", "swap": "ss2dc16s", "deep": "ss2dc16"}[kind]
        assert {fam + "_fwd", fam + "_bwd"} <= ran, sorted(ran)
        assert not ({"ss2d_fwd", "ss2d_bwd", "cross_scan", "selective_scan_fwd", "dt_proj_fwd"} & ran), sorted(ran)


@pytest.mark.parametrize("cfg,node", [tuple(i.split("-")) for i in NODE_IDS], ids=NODE_IDS)
def test_ss2d_node_at_the_production_shape_matches_the_oracle(cfg, node):
    kind, Bt, D, HW, R, N = _node_table(cfg)[node]
    (x, xw, dtw, A, Dp, bias, gy), got, ran, ws_seen = _run_node(cfg, node)
    _check_plan(cfg, node, ran, ws_seen)
    ref = _oracle_full(kind, Bt, HW, N, x, xw, dtw, A, Dp, bias, gy)
    # y: 2e-3 of the scale where test_hip_chan.py holds the channel-lane kernels to it (maps up to 12 x 12), 5e-3 at 14 x 14
    # (bf16 partial-sum planes); the wide-map kernels and the operator chain (bf16 step sizes between two launches) at
    # BASELINE's 1e-2 for bf16 I/O, as test_hip_ops.py does
    ytol = 1e-2 if kind == "wide" or (kind == "swap" and not _swap_kernel_covers(cfg)) else (5e-3 if HW > 12 else 2e-3)
    # per-sample tensors on EVERY sample (all XCD slots of the sample maps), batch sums over the whole batch
    for name, a, b, tol in zip(("y", "dx", "dx_proj_w", "ddt_w", "dA", "dD", "dbias"), got, ref, (ytol,) + (1e-2,) * 6):
        b = b.float().reshape(a.shape)
        assert_close(a, b, tol, tol * float(b.abs().max()) + 1e-7, f"{cfg} {node} {name}")


XMAP_CASES = [("small", "s1"), ("small", "s2"), ("base384", "s1"), ("base384", "s3")]


def _child_run_node(cfg, node, path):
    """Entry of the child process of the XCD-map test (a fresh process: the switches are read once per process)."""
    _, got, ran, ws_seen = _run_node(cfg, node)
    torch.save({"got": got, "ran": sorted(ran), "ws": ws_seen}, path)


def _in_child(env, code, timeout):
    e = dict(os.environ, **env)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.mark.parametrize("cfg,node", XMAP_CASES, ids=[f"{c}-{n}" for c, n in XMAP_CASES])
def test_xcd_sample_map_does_not_change_results(cfg, node, tmp_path):
    """One wide-map node and one channel-lane node per model with the XCD-local sample map switched off (XFM_L3_NO_XMAP /
    XFM_CHAN_NO_XMAP) in a child process: the same results to 2e-3 of each tensor's scale, so a wrong sample placement in
    the map cannot hide behind the oracle tolerance of the node tests."""
    kind, Bt = _node_table(cfg)[node][:2]
    assert Bt % 8 == 0                                   # (the map is on at the default run)
    _, ref, _, _ = _run_node(cfg, node)
    var = "XFM_L3_NO_XMAP" if kind == "wide" else "XFM_CHAN_NO_XMAP"
    out = tmp_path / "node.pt"
    _in_child({var: "1"}, f"from tests.test_hip_configs import _child_run_node; _child_run_node({cfg!r}, {node!r}, {str(out)!r})", 900)
    got = torch.load(out)["got"]
    for name, a, b in zip(("y", "dx", "dx_proj_w", "ddt_w", "dA", "dD", "dbias"), got, ref):
        assert_close(a, b, 2e-3, 2e-3 * float(b.abs().max()) + 1e-7, f"{cfg} {node} {name} without the sample map")


def test_plan_assertions_see_the_kernel_switches(monkeypatch):
    """The plan assertions are not vacuous: with the wide-map kernels' dB / dC sums moved to atomics (XFM_L3_ATOMICS, read per
    call) the workspace check fails, and with the fourth-generation kernels off (XFM_SS2D_W=0, read once per process: a
    child process) XFMamba-B's 48 x 48 node no longer reads fp32 B / C rows."""
    from xfmamba_amd import _lib
    monkeypatch.setenv("XFM_L3_ATOMICS", "1")
    _, _, ran, ws_seen = _run_node("small", "s1")
    with pytest.raises(AssertionError):
        _check_plan("small", "s1", ran, ws_seen)
    monkeypatch.delenv("XFM_L3_ATOMICS")
    _, Bt, D, HW, _, N = _node_table("base384")["s1"]
    q = f"from xfmamba_amd import _lib; print(_lib.lib().xfm_ss2d_bc_f32({Bt}, {D}, {HW}, {HW}, {N}, {_lib.dtype_code(torch.bfloat16)}))"
    assert _lib.lib().xfm_ss2d_bc_f32(Bt, D, HW, HW, N, _lib.dtype_code(torch.bfloat16)) == 1
    assert _in_child({"XFM_SS2D_W": "0"}, q, 300).strip().splitlines()[-1] == "0"


# ---------------------------------------------------------------------------------------------------------------------------
# Part 2: the whole models at the bench batch
# ---------------------------------------------------------------------------------------------------------------------------

# checked samples: several residues b % 8 (XCD slots of the sample maps; after the view merge sample b is also row B + b)
PICK = {"small": [0, 9, 18, 31], "base384": [3, 12]}


@pytest.mark.parametrize("cfg", ["small", "base384"])
def test_model_bf16_at_the_bench_batch_matches_oracle_samples(cfg):
    """Eval forward of the whole model under bf16 autocast at the per-GPU bench batch (32 / 16 two-view samples in one pass;
    BatchNorm on running statistics, so the samples are independent).  The picked samples against the CPU oracle: fp32 =
    truth, oracle under bf16 autocast = yardstick, d_hip <= 1.5 d_orc + 2e-3 and below the 3e-2 cap (the rule of
    test_model_tiny_bf16_at_the_bench_batch_matches_oracle_samples)."""
    (_, ty, kw, size, _), batch = BENCH[cfg]
    m = _model_with_synth_weights(ty, kw).eval()
    g = torch.Generator().manual_seed(42)
    xa, xb = torch.randn(batch, 1, size, size, generator=g), torch.randn(batch, 1, size, size, generator=g)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        logits = m(xa.to(DEV), xb.to(DEV)).float().cpu()
    del m
    pick = torch.tensor(PICK[cfg])
    sd = O.synth_state_dict(load_json("g5_state_shapes.json")[ty], seed=0)
    with torch.no_grad():
        ref = O.xfmamba_top_ref(sd, xa[pick], xb[pick], False, c_scan.selective_scan_c).float()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            lo = O.xfmamba_top_ref(sd, xa[pick], xb[pick], False, c_scan.selective_scan_c).float()
    scale = float(ref.abs().max())
    d_orc = float((lo - ref).abs().max()) / scale
    d_hip = float((logits[pick] - ref).abs().max()) / scale
    assert 1e-3 < d_orc < 3e-2, d_orc
    assert d_hip <= 1.5 * d_orc + 2e-3, (d_hip, d_orc)
    assert d_hip < 3e-2, d_hip
    # the other samples went through the same launches: finite, and the batch is not a broadcast of one sample
    assert torch.isfinite(logits).all() and float(logits.std(0).min()) > 0


@pytest.mark.parametrize("cfg", ["small", "base384"])
def test_model_bf16_bench_batch_training_gradients_match_the_oracle_on_picked_samples(cfg):
    """Training backward of the whole model under bf16 autocast at the per-GPU bench batch (DropPath 0, BatchNorm on running
    statistics: the samples do not interact).  The full batch runs forward; the cotangent -- d CE / d logits at the fp32
    oracle's logits -- flows back through the picked samples' logits only, so the parameter gradients are those of the picked
    samples, which the CPU oracle computes (fp32 = truth, bf16 autocast with bf16 scan operands = yardstick).  Every gradient
    norm within 1.5x the yardstick's error + 5e-2, the global norm within 1.5x + 1e-2, sampled tensors of every stage and both
    fusion blocks in direction (the rule of test_model_tiny_bf16_batch32_training_gradients_match_the_oracle_on_four_samples)."""
    from xfmamba_amd import _lib
    (_, ty, kw, size, _), batch = BENCH[cfg]
    g = torch.Generator().manual_seed(4321)
    xa, xb = torch.randn(batch, 1, size, size, generator=g), torch.randn(batch, 1, size, size, generator=g)
    lab = torch.randint(0, 2, (batch,), generator=g)
    pick = torch.tensor(PICK[cfg])
    sd = O.synth_state_dict(load_json("g5_state_shapes.json")[ty], seed=0)
    cot = {}

    def oracle_grads(autocast):
        leaves = {k: v.clone().requires_grad_(v.is_floating_point() and "running_" not in k) for k, v in sd.items()}
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            o = O.xfmamba_top_ref(leaves, xa[pick], xb[pick], False, bf16_operand_scan if autocast else c_scan.selective_scan_c)
        if "g" not in cot:
            lg = o.detach().float().requires_grad_()
            torch.nn.functional.cross_entropy(lg, lab[pick]).backward()
            cot["g"] = lg.grad.clone()
        o.float().backward(cot["g"])
        return {k: v.grad.float() for k, v in leaves.items() if v.requires_grad and v.grad is not None}, o.detach().float()

    ref, lo_ref = oracle_grads(False)
    orc, _ = oracle_grads(True)
    m = _model_with_synth_weights(ty, kw).train()
    for mod in m.modules():
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    timer = _lib.KernelTimer()
    _lib.set_timer(timer)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(xa.to(DEV), xb.to(DEV))
        out.float()[pick.to(DEV)].backward(cot["g"].to(DEV))
        ran = set(timer.summary())
    finally:
        _lib.set_timer(None)
    want = {"ss2d_fwd", "ss2d_bwd", "ss2dc_fwd", "ss2dc_bwd", "ss2dc16_fwd", "ss2dc16_bwd"}
    if _swap_kernel_covers(cfg):
        want |= {"ss2dc16s_fwd", "ss2dc16s_bwd"}
        assert not ({"selective_scan_fwd", "selective_scan_bwd"} & ran), sorted(ran)
    else:                                          # (the shallow block of XFMamba-B@384 runs the operator chain)
        want |= {"selective_scan_fwd", "selective_scan_bwd"}
    assert want <= ran and "cross_scan" not in ran, sorted(ran)
    hip = {k: p.grad.float().cpu() for k, p in m.named_parameters() if p.grad is not None}
    assert torch.isfinite(out).all()
    d_log = float((out.detach().float().cpu()[pick] - lo_ref).abs().max()) / float(lo_ref.abs().max())
    assert d_log < 3e-2, d_log
    assert set(ref) == set(hip), set(ref) ^ set(hip)
    sampled = [k for pat in ("patch_embed.0.weight", "layers.0.blocks.0.op.x_proj_weight", "layers.0.blocks.1.op.dt_projs_weight",
                             "layers.1.blocks.0.op.A_logs", "layers.1.blocks.1.op.x_proj_weight", "layers.2.blocks.3.mlp.fc1.weight",
                             "layers.2.blocks.7.op.out_proj.weight", "layers.2.blocks.0.op.dt_projs_weight",
                             "layers.3.blocks.1.op.in_proj.weight", "layers.3.blocks.0.op.x_proj_weight",
                             "shallowfuseSS2D.x_proj_weight", "shallowfuseSS2D.dt_projs_weight",
                             "fusemamba.blocks.0.self_attention.x_proj_weight", "fusemamba.blocks.0.self_attention.dt_projs_weight",
                             "final_conv")
               for k in sorted(ref) if pat in k]
    for pat in ("layers.0.", "layers.1.", "layers.2.", "layers.3.", "shallowfuseSS2D", "fusemamba"):
        assert any(pat in k for k in sampled), (pat, sampled)
    tot_h = tot_o = tot_r = 0.0
    for k, gr in ref.items():
        rn = float(gr.double().norm())
        eh = abs(float(hip[k].double().norm()) - rn) / (rn + 1e-12)
        eo = abs(float(orc[k].double().norm()) - rn) / (rn + 1e-12)
        if gr.numel() < 16:
            # (the classifier's 2-element bias gradient: a cancelling sum of O(1) terms, held element-wise as in the T test)
            da, do = float((hip[k] - gr).abs().max()), float((orc[k] - gr).abs().max())
            assert da <= 1.5 * do + 2e-2, (k, da, do)
        else:
            assert eh <= 1.5 * eo + 5e-2, (k, eh, eo)
        tot_h += float(hip[k].double().pow(2).sum()); tot_o += float(orc[k].double().pow(2).sum()); tot_r += rn * rn
        if k in sampled and rn > 0:
            cos = float(torch.nn.functional.cosine_similarity(hip[k].flatten().double(), gr.flatten().double(), dim=0))
            cos_o = float(torch.nn.functional.cosine_similarity(orc[k].flatten().double(), gr.flatten().double(), dim=0))
            assert cos > min(0.97, cos_o - 0.02), (k, cos, cos_o)
    eh, eo = abs(tot_h ** 0.5 - tot_r ** 0.5) / tot_r ** 0.5, abs(tot_o ** 0.5 - tot_r ** 0.5) / tot_r ** 0.5
    assert eh <= 1.5 * eo + 1e-2, (eh, eo)
