"""`altcorr` operator surface (names of cdvslam/altcorr/correlation.py:51-75) on the HIP kernels.  Without autograd the
forward takes the fast / fused paths; with grad enabled and a differentiable input it goes through the autograd
Functions below (CorrLayer / PatchLayer of the reference), whose backward passes are cdv_corr_bwd / cdv_patchify_bwd."""
import torch

from .. import ops

_MODES = ("bilinear", "upperleft")


def _differentiable(*ts):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in ts)


class _CorrLayer(torch.autograd.Function):
    """CorrLayer (correlation.py:4-30): the generic planar forward, the HIP backward on a dropout subset of the edges"""

    @staticmethod
    def forward(ctx, fmap1, fmap2, coords, ii, jj, radius, dropout):
        ctx.save_for_backward(fmap1, fmap2, coords, ii, jj)
        ctx.radius, ctx.dropout = radius, dropout
        return ops.corr_forward_plain(fmap1, fmap2, coords, ii, jj, radius)

    @staticmethod
    def backward(ctx, grad):
        fmap1, fmap2, coords, ii, jj = ctx.saved_tensors
        if ctx.dropout < 1:
            # one draw of length M per backward, as the reference (correlation.py:20-25)
            keep = torch.rand(len(ii), device=grad.device) < ctx.dropout
            coords, grad, ii, jj = coords[:, keep], grad[:, keep], ii[keep], jj[keep]
        g1, g2 = ops.corr_backward(fmap1, fmap2, coords, ii, jj, grad, ctx.radius, need=ctx.needs_input_grad[:2])
        return g1, g2, None, None, None, None, None


class _PatchLayer(torch.autograd.Function):
    """PatchLayer (correlation.py:33-48): the raw (2r+2)^2 gather and its adjoint"""

    @staticmethod
    def forward(ctx, net, coords, radius):
        ctx.save_for_backward(net, coords)
        ctx.radius = radius
        return ops.patchify_forward(net, coords, radius)

    @staticmethod
    def backward(ctx, grad):
        net, coords = ctx.saved_tensors
        g = ops.patchify_backward(net, coords, grad, ctx.radius) if ctx.needs_input_grad[0] else None
        return g, None, None


def corr(fmap1, fmap2, coords, ii, jj, radius=1, dropout=1):
    """Local correlation volume + bilinear blend (correlation.py:74-75 -> CorrLayer.forward :6-13).
    Returns [B, M, 2r+1 (x), 2r+1 (y), P, P].  Differentiable in fmap1 and fmap2 (float32 maps); `dropout` < 1 keeps
    that fraction of the edges in the backward, as the reference."""
    if _differentiable(fmap1, fmap2):
        return _CorrLayer.apply(fmap1, fmap2, coords, ii, jj, radius, dropout)
    return ops.corr_forward(fmap1, fmap2, coords, ii, jj, radius)


def patchify(net, coords, radius, mode='bilinear'):
    """(2r+1)^2 samples around coords [B,M,2] of net [B,C,H,W] (correlation.py:51-71): 'bilinear' blends the four
    neighbouring gathers (float32 result), 'upperleft' keeps the one sample at floor(coords), any other mode returns
    the raw (2r+2)^2 gather.  Without autograd gather and blend are one launch (cdv_patchify_blend / cdv_patchify_fwd);
    with grad enabled and net or coords requiring grad, the raw gather is a Function and the mode's torch expression
    follows, as in the reference (so 'bilinear' differentiates in coords too)."""
    if _differentiable(net, coords):
        patches = _PatchLayer.apply(net, coords, radius)
        if mode == 'bilinear':
            offset = (coords - coords.floor()).to(net.device)
            dx, dy = offset[:, :, None, None, None].unbind(dim=-1)
            d = 2 * radius + 1
            x00 = (1 - dy) * (1 - dx) * patches[..., :d, :d]
            x01 = (1 - dy) * dx * patches[..., :d, 1:]
            x10 = dy * (1 - dx) * patches[..., 1:, :d]
            x11 = dy * dx * patches[..., 1:, 1:]
            return x00 + x01 + x10 + x11
        if mode == 'upperleft':
            return patches[..., :1, :1]
        return patches
    if mode in _MODES:
        return ops.patchify_blend(net, coords, radius, mode)
    return ops.patchify_forward(net, coords, radius)
