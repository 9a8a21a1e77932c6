"""``cross_scan_fn`` / ``cross_merge_fn`` and the two-view swap -- drop-ins for the reference.

Mirrors ``models/csm_triton.py:501-517`` (dispatchers), ``:182-273`` (CrossScanF/CrossMergeF
autograd pairing: the backward of a scan is a merge and vice versa) and
``models/fusion_vmamba.py:189-241`` (SwappingScan_multiview / SwappingMerge_multiview) of
XZheng0427/XFMamba.  Every configuration of the reference's ``triton_cross_scan_flex``
(``models/csm_triton.py:279-400``) is built: channel-first or channel-last x and y, ``one_by_one``,
and ``scans`` 0 (cross2d), 1 (unidirectional) and 2 (bidirectional); SURVEY.md section 8 row a2.
The hot-path configuration (``scans=0``, channel-first in and out, ``one_by_one=False``) runs the
``xfm_cross_scan`` / ``xfm_cross_merge`` kernels, every other one ``xfm_cross_scan_flex`` /
``xfm_cross_merge_flex``.  The cascade mode ``scans=-1`` and ``force_torch=True`` raise
``NotImplementedError``; there is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib

__all__ = ["cross_scan_fn", "cross_merge_fn", "CrossScanHip", "CrossMergeHip", "CrossScanFlexHip", "CrossMergeFlexHip",
           "SwappingScan_multiview", "SwappingMerge_multiview", "SwappingScanStacked"]


def _scan(x: torch.Tensor) -> torch.Tensor:
    _lib.require_cuda(x)
    B, C, H, W = x.shape
    x = x.contiguous()
    y = torch.empty((B, 4, C, H * W), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _lib.timed("cross_scan", 5 * x.numel() * x.element_size()):
        _lib.check(_lib.lib().xfm_cross_scan(x.data_ptr(), y.data_ptr(), B, C, H, W, _lib.dtype_code(x.dtype),
                                             _lib.stream_ptr()), "cross_scan")
    return y


def _merge(ys: torch.Tensor, H: int, W: int, out_dtype=None) -> torch.Tensor:
    _lib.require_cuda(ys)
    B, K, C = ys.shape[0], ys.shape[1], ys.shape[2]
    assert K == 4
    ys = ys.contiguous()
    out_dtype = out_dtype or ys.dtype
    x = torch.empty((B, C, H * W), dtype=out_dtype, device=ys.device)
    with torch.cuda.device(ys.device), _lib.timed("cross_merge", ys.numel() * ys.element_size() + x.numel() * x.element_size()):
        _lib.check(_lib.lib().xfm_cross_merge(ys.data_ptr(), x.data_ptr(), B, C, H, W, _lib.dtype_code(ys.dtype),
                                              _lib.dtype_code(out_dtype), _lib.stream_ptr()), "cross_merge")
    return x


class CrossScanHip(torch.autograd.Function):
    """(B, C, H, W) -> (B, 4, C, H*W); backward = cross merge (csm_triton.py:207-225)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor):
        ctx.hw = x.shape[2:]
        return _scan(x)

    @staticmethod
    def backward(ctx, ys: torch.Tensor):
        H, W = ctx.hw
        B, K, C, L = ys.shape
        return _merge(ys, H, W).view(B, C, H, W)


class CrossMergeHip(torch.autograd.Function):
    """(B, 4, C, H, W) -> (B, C, H*W); backward = cross scan (csm_triton.py:248-273)."""

    @staticmethod
    def forward(ctx, ys: torch.Tensor):
        B, K, C, H, W = ys.shape
        ctx.shape = (B, C, H, W)
        return _merge(ys, H, W)

    @staticmethod
    def backward(ctx, x: torch.Tensor):
        B, C, H, W = ctx.shape
        return _scan(x.reshape(B, C, H, W)).view(B, 4, C, H, W)


def _scan_flex(x: torch.Tensor, B, C, H, W, in_cf, out_cf, obo, scans) -> torch.Tensor:
    x = x.contiguous()
    L = H * W
    y = x.new_empty((B, 4, C, L) if out_cf else (B, L, 4, C))
    with torch.cuda.device(x.device), _lib.timed("cross_scan_flex", 5 * x.numel() * x.element_size() if not obo
                                                 else 2 * x.numel() * x.element_size()):
        _lib.check(_lib.lib().xfm_cross_scan_flex(x.data_ptr(), y.data_ptr(), B, C, H, W, int(not in_cf), int(not out_cf),
                                                  int(obo), scans, _lib.dtype_code(x.dtype), _lib.stream_ptr()),
                   "cross_scan_flex")
    return y


def _merge_flex(y: torch.Tensor, B, C, H, W, in_cf, out_cf, obo, scans) -> torch.Tensor:
    y = y.contiguous()
    L = H * W
    if obo:
        x = y.new_empty((B, 4, C, L) if in_cf else (B, L, 4, C))
    else:
        x = y.new_empty((B, C, L) if in_cf else (B, L, C))
    with torch.cuda.device(y.device), _lib.timed("cross_merge_flex", y.numel() * y.element_size() + x.numel() * x.element_size()):
        _lib.check(_lib.lib().xfm_cross_merge_flex(y.data_ptr(), x.data_ptr(), B, C, H, W, int(not in_cf), int(not out_cf),
                                                   int(obo), scans, _lib.dtype_code(y.dtype), _lib.dtype_code(y.dtype),
                                                   _lib.stream_ptr()), "cross_merge_flex")
    return x


def _x_shape(B, C, H, W, in_cf, obo):
    if obo:
        return (B, 4, C, H, W) if in_cf else (B, H, W, 4, C)
    return (B, C, H, W) if in_cf else (B, H, W, C)


class CrossScanFlexHip(torch.autograd.Function):
    """Every other configuration of CrossScanTritonF (csm_triton.py:403-453): x (B, C, H, W) | (B, H, W, C) |
    (B, 4, C, H, W) | (B, H, W, 4, C) -> y (B, 4, C, H*W) | (B, H*W, 4, C); backward = the merge with the same flags."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, in_cf: bool, out_cf: bool, obo: bool, scans: int):
        if obo:
            B, _, C, H, W = x.shape if in_cf else (x.shape[0], None, x.shape[4], x.shape[1], x.shape[2])
        else:
            B, C, H, W = x.shape if in_cf else (x.shape[0], x.shape[3], x.shape[1], x.shape[2])
        ctx.cfg = (B, C, H, W, in_cf, out_cf, obo, scans)
        return _scan_flex(x, *ctx.cfg)

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        B, C, H, W, in_cf, out_cf, obo, scans = ctx.cfg
        return _merge_flex(gy, *ctx.cfg).view(_x_shape(B, C, H, W, in_cf, obo)), None, None, None, None


class CrossMergeFlexHip(torch.autograd.Function):
    """Every other configuration of CrossMergeTritonF (csm_triton.py:456-498): y (B, 4, C, H, W) | (B, H, W, 4, C) ->
    x (B, C, H*W) | (B, H*W, C) | (B, 4, C, H*W) | (B, H*W, 4, C); backward = the scan with the same flags.
    As in the reference, ``in_cf`` describes the merge's output x and ``out_cf`` its input y."""

    @staticmethod
    def forward(ctx, y: torch.Tensor, in_cf: bool, out_cf: bool, obo: bool, scans: int):
        if out_cf:
            B, _, C, H, W = y.shape
        else:
            B, H, W, _, C = y.shape
        ctx.cfg = (B, C, H, W, in_cf, out_cf, obo, scans)
        return _merge_flex(y, *ctx.cfg)

    @staticmethod
    def backward(ctx, gx: torch.Tensor):
        B, C, H, W, in_cf, out_cf, obo, scans = ctx.cfg
        gy = _scan_flex(gx, *ctx.cfg)
        return gy.view((B, 4, C, H, W) if out_cf else (B, H, W, 4, C)), None, None, None, None


def _route_config(t: torch.Tensor, in_channel_first, out_channel_first, one_by_one, scans, force_torch) -> bool:
    """True for the hot-path configuration (the xfm_cross_scan / xfm_cross_merge kernels)."""
    if force_torch:
        raise NotImplementedError("force_torch: the torch implementation is test infrastructure (oracle/), not shipped")
    if scans not in (0, 1, 2):
        raise NotImplementedError(f"scans={scans!r}: xfmamba_amd builds cross2d (0), unidirectional (1) and "
                                  f"bidirectional (2) routes; the cascade mode (-1) is not built")
    hot = bool(in_channel_first) and bool(out_channel_first) and not one_by_one and scans == 0
    if not hot and not t.is_cuda:
        raise NotImplementedError("xfmamba_amd: operands must live on an MI355X device (no CPU path; "
                                  "the CPU oracle under oracle/ is test infrastructure only)")
    return hot


def cross_scan_fn(x: torch.Tensor, in_channel_first=True, out_channel_first=True, one_by_one=False, scans=0,
                  force_torch=False):
    """Same signature as the reference (models/csm_triton.py:501-507)."""
    if _route_config(x, in_channel_first, out_channel_first, one_by_one, scans, force_torch):
        return CrossScanHip.apply(x)
    return CrossScanFlexHip.apply(x, bool(in_channel_first), bool(out_channel_first), bool(one_by_one), int(scans))


def cross_merge_fn(y: torch.Tensor, in_channel_first=True, out_channel_first=True, one_by_one=False, scans=0,
                   force_torch=False):
    """Same signature as the reference (models/csm_triton.py:511-517)."""
    if _route_config(y, in_channel_first, out_channel_first, one_by_one, scans, force_torch):
        return CrossMergeHip.apply(y)
    return CrossMergeFlexHip.apply(y, bool(in_channel_first), bool(out_channel_first), bool(one_by_one), int(scans))


class SwappingScan_multiview(torch.autograd.Function):
    """Even channels exchanged between the two views -> (B, 2, C, H*W).

    The backward is the reference's un-swapped pass-through (fusion_vmamba.py:217-221), kept
    bit-for-meaning: it is NOT the adjoint of the forward."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, x2: torch.Tensor):
        _lib.require_cuda(x, x2)
        B, C, H, W = x.shape
        ctx.shape = (B, C, H, W)
        x, x2 = x.contiguous(), x2.contiguous()
        out = torch.empty((B, 2, C, H * W), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().xfm_swap_scan(x.data_ptr(), x2.data_ptr(), out.data_ptr(), B, C, H * W,
                                                _lib.dtype_code(x.dtype), _lib.stream_ptr()), "swap_scan")
        return out

    @staticmethod
    def backward(ctx, ys: torch.Tensor):
        B, C, H, W = ctx.shape
        return ys[:, 0].reshape(B, -1, H, W), ys[:, 1].reshape(B, -1, H, W)


class SwappingScanStacked(torch.autograd.Function):
    """``SwappingScan_multiview`` on the two views stacked along the batch axis, ``x`` = [view 1 | view 2] (2B, C, H, W) ->
    (B, 2, C, H*W).  Same forward kernel and the same pass-through backward (fusion_vmamba.py:217-221: route k's gradient
    goes to view k un-swapped), returned as ONE (2B, C, H, W) tensor instead of two slice gradients."""

    @staticmethod
    def forward(ctx, x: torch.Tensor):
        _lib.require_cuda(x)
        B2, C, H, W = x.shape
        B = B2 // 2
        ctx.shape = (B, C, H, W)
        x = x.contiguous()
        out = torch.empty((B, 2, C, H * W), dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().xfm_swap_scan(x.data_ptr(), x[B:].data_ptr(), out.data_ptr(), B, C, H * W,
                                                _lib.dtype_code(x.dtype), _lib.stream_ptr()), "swap_scan")
        return out

    @staticmethod
    def backward(ctx, ys: torch.Tensor):
        B, C, H, W = ctx.shape
        return ys.transpose(0, 1).reshape(2 * B, C, H, W)


class SwappingMerge_multiview(torch.autograd.Function):
    """(B, 2, C, L) -> two (B, C, L) tensors, no un-swap (fusion_vmamba.py:224-241)."""

    @staticmethod
    def forward(ctx, ys: torch.Tensor):
        return ys[:, 0].contiguous(), ys[:, 1].contiguous()

    @staticmethod
    def backward(ctx, x: torch.Tensor, x2: torch.Tensor):
        return torch.stack([x, x2], dim=1)
