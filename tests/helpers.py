"""Shared helpers for the parity tests."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def load_npz(name):
    return np.load(os.path.join(GOLDEN, name))


def load_json(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def g1_case_tensors(z, case):
    """Rebuild the typed input tensors of a g1 case from the stored fp32 arrays."""
    name, dt = case[0], _DT[case[10]]
    t = {}
    for k in ("u", "delta", "A", "B", "C", "D", "delta_bias", "dout"):
        key = f"{name}/in/{k}"
        t[k] = torch.from_numpy(z[key]) if key in z.files else None
    for k in ("u", "delta", "B", "C"):
        t[k] = t[k].to(dt)
    return t


def max_rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def assert_close(a, b, rtol, atol, what=""):
    a, b = a.double(), b.double()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: max abs err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e}), " \
                                f"{int(bad.sum())}/{bad.numel()} outside rtol={rtol} atol={atol}"


# ---- whole-model helpers shared by test_hip_model.py and test_hip_configs.py

# BASELINE.json model sizes: (golden tag, type, ctor kwargs, image size, batch) -- net_fusionmamba.py:150-159
MODEL_CFGS = {
    "tiny": ("g5", "tiny", {}, 224, 2),                                   # configs[0]/[1]
    "small": ("g5s", "small", {}, 224, 2),                                # configs[2]
    "base384": ("g5b", "base", dict(hidden_dim=1024), 384, 1),            # configs[3]
}


def _model_with_synth_weights(ty="tiny", kw=None, device="cuda"):
    from oracle import xfm_oracle as O
    from xfmamba_amd.net_fusionmamba import TwoViewXFMambaTop
    shapes = load_json("g5_state_shapes.json")[ty]
    m = TwoViewXFMambaTop(in_channels=1, outputs=2, type=ty, **(kw or {}))
    m.load_state_dict(O.synth_state_dict(shapes, seed=0), strict=True)
    return m.to(device)


def bf16_operand_scan(u, delta, A, B, C, *rest):
    """The CPU scan with its x / delta / B / C operands rounded to bf16 (straight-through: the gradient passes unchanged) --
    the precision the HIP scan reads them in under bf16 autocast; A, D and the bias stay fp32 as they do there.  (Under CPU
    autocast the oracle's operands arrive in bf16 already; the rounding states that precision instead of relying on which
    operators autocast lowers, and hands the scan fp32 tensors either way.)"""
    from oracle import c_scan

    def st(t):
        t = t.float()
        return t + (t.bfloat16().float() - t).detach()
    return c_scan.selective_scan_c(st(u), st(delta), A, st(B), st(C), *rest)


def _oracle_autocast_grads(ty_tag, sd, xa, xb, lab):
    """Gradients of the CPU oracle under bf16 autocast (same GEMM precision as the bench configuration, fp32 scan state on
    bf16-rounded scan operands): the yardstick for what bf16 arithmetic itself does to the gradients."""
    from oracle import xfm_oracle as O
    leaves = {k: v.clone().requires_grad_(v.is_floating_point() and "running_" not in k) for k, v in sd.items()}
    with torch.autocast("cpu", dtype=torch.bfloat16):
        out = O.xfmamba_top_ref(leaves, xa, xb, True, bf16_operand_scan)
    torch.nn.functional.cross_entropy(out.float(), lab).backward()
    return {k: v.grad for k, v in leaves.items() if v.requires_grad and v.grad is not None}
