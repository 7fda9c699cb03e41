"""`projective_ops` operator surface (names and argument meaning of cdvslam/projective_ops.py) on the fused HIP kernels.

`transform` (+ validity, Jacobians, translation-only), `flow_mag` and `point_cloud` are ONE launch each
(cdv_transform / cdv_flow_mag / cdv_point_cloud) where the reference composes gathers, lietorch Inv / Mul / Act4 and
elementwise ops (projective_ops.py:53-130).  The kernels serve what the update path hands them -- float32 state, batch
1, SE3 poses -- and anything else raises: there is no composed fallback.  `iproj` / `proj` are the two pinhole maps as
plain tensor expressions for callers that want them on their own.

Autograd.  With grad mode on and poses (the tensor, or a group object's `.data`) or patches that require grad, `transform`
runs through `_TransformFn`: the forward is the same launch (`ops.transform`, the same bits, the same permuted view of an
E2PP buffer), the backward is `ops.transform_backward` (csrc/transform_bwd.hip) -- the pose gradient is the
left-perturbation row vector the Lie classes and the reference's GroupOps exchange.  Otherwise a call is exactly the code
path without autograd, the compiled lane included.  The intrinsics carry no gradient and `tonly=True` has no backward
(NotImplementedError for both).  ONE branch is composed instead of fused: `jacobian=True` under grad (the reference's ba.py
reaches it from its second iteration on with poses that require grad).  There the coordinates and `valid` still come from
the fused Function, but the Jacobians carry gradient in the reference and there are no fused second derivatives here, so
(Ji, Jj, Jz) are built by `_jacobians_composed` from this package's differentiable Lie classes with the reference's formulas
(projective_ops.py:71-106).  `reproject`, `flow_mag` and `point_cloud` are inference only: they return tensors without a
graph.
"""
import torch

from . import ops

MIN_DEPTH = 0.2


def _fc(intrinsics):
    """[b,n,4] -> focal lengths and principal point as [b,n,2,1,1] each"""
    k = intrinsics[..., None, None]
    return k[:, :, 0:2], k[:, :, 2:4]


def iproj(patches, intrinsics):
    """pixel grid + inverse depth -> homogeneous rays: patches [b,n,3,P,P], intrinsics [b,n,4] -> [b,n,P,P,4]
    (x - cx) / fx, (y - cy) / fy, 1, d    (projective_ops.py:19-29)"""
    f, c = _fc(intrinsics)
    rays = (patches[:, :, 0:2] - c) / f
    d = patches[:, :, 2:3]
    return torch.cat([rays, torch.ones_like(d), d], dim=2).movedim(2, -1)


def proj(X, intrinsics, depth=False):
    """homogeneous points [b,n,P,P,4] -> pixels [b,n,P,P,2] (or 3 with the inverse depth), 1 / max(Z, 0.1) as the
    reference clamps it (projective_ops.py:32-50)"""
    f, c = _fc(intrinsics)
    inv_z = X[..., 2].clamp(min=0.1).reciprocal()
    uv = f.movedim(2, -1) * (X[..., 0:2] * inv_z[..., None]) + c.movedim(2, -1)
    return torch.cat([uv, inv_z[..., None]], dim=-1) if depth else uv


def _kernel_pose_rows(poses, what):
    """the [1,n,7] float32 tensor the kernels read, or an error naming what is not served"""
    # a tensor, this package's LieGroup, or the caller's own group object (the reference's lietorch.SE3 when only
    # projective_ops is substituted, install_dropin(package=)): anything that carries its rows in `.data` and names its group
    group = not torch.is_tensor(poses)
    data = getattr(poses, "data", None) if group else poses
    if group and getattr(poses, "group_id", None) != 3:
        raise NotImplementedError("%s: SE3 poses only (Sim3 belongs to loop closure, out of scope)" % what)
    if not torch.is_tensor(data):
        raise TypeError("%s: poses must be an SE3 or a tensor" % what)
    if data.dtype != torch.float32 or data.dim() != 3 or data.shape[0] != 1:
        raise NotImplementedError("%s: the HIP path serves float32 poses of batch 1 (got %s %s); no composed fallback"
                                  % (what, data.dtype, tuple(data.shape)))
    return data


class _TransformFn(torch.autograd.Function):
    """coords [1,E,P,P,2] (and the per-pixel validity mask) of the fused transform with the fused backward: the launches and
    the layouts of the call without autograd"""

    @staticmethod
    def forward(ctx, data, patches, intrinsics, ii, jj, kk, valid):
        ctx.save_for_backward(data, patches, intrinsics, ii, jj, kk)
        if valid:
            coords, mask = ops.transform(data, patches, intrinsics, ii, jj, kk, layout_e2pp=False, valid=True)
            ctx.mark_non_differentiable(mask)
            return coords, mask
        return ops.transform(data, patches, intrinsics, ii, jj, kk, layout_e2pp=True).permute(0, 1, 3, 4, 2), None

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad, _grad_mask):
        data, patches, intrinsics, ii, jj, kk = ctx.saved_tensors
        # what comes back through the caller's `.permute(0, 1, 4, 2, 3).contiguous()` is a permuted view of a contiguous
        # [1,E,2,P,P] buffer: transform_backward reads it where it lies
        dposes, dpatches = ops.transform_backward(data, patches, intrinsics, ii, jj, kk, grad, need=ctx.needs_input_grad[0:2])
        return dposes, dpatches, None, None, None, None, None


def _jacobians_composed(poses, patches, intrinsics, ii, jj, kk):
    """(Ji, Jj, Jz) of the reference's formulas (projective_ops.py:71-106) over this package's differentiable Lie classes, in
    the dtype of its inputs (a float64 run of this function is the truth of its float32 run).  poses: an SE3 of this
    package.  The last column of Gij.matrix() is Gij * (0, 0, 0, 1) (act4): as_matrix has no backward here."""
    P = patches.shape[-1]
    c = P // 2
    Gij = poses[:, jj] * poses[:, ii].inv()
    X0 = iproj(patches[:, kk][..., c:c + 1, c:c + 1], intrinsics[:, ii])[:, :, 0, 0]          # the centre pixel, [1,E,4]
    X, Y, Z, H = (Gij * X0).unbind(dim=-1)
    o = torch.zeros_like(H)
    fx, fy, _, _ = intrinsics[:, jj].unbind(dim=-1)
    far = Z.abs() > 0.2
    d = torch.where(far, 1.0 / torch.where(far, Z, torch.ones_like(Z)), o)
    Ja = torch.stack([H, o, o, o, Z, -Y,
                      o, H, o, -Z, o, X,
                      o, o, H, Y, -X, o,
                      o, o, o, o, o, o], dim=-1).view(1, len(ii), 4, 6)
    Jp = torch.stack([fx * d, o, -fx * X * d * d, o,
                      o, fy * d, -fy * Y * d * d, o], dim=-1).view(1, len(ii), 2, 4)
    Jj = torch.matmul(Jp, Ja)
    Ji = -Gij[:, :, None].adjT(Jj)
    e4 = torch.zeros_like(X0)
    e4[..., 3] = 1.0
    Jz = torch.matmul(Jp, (Gij * e4)[..., None])
    return Ji, Jj, Jz


def _transform_grad(poses, data, patches, intrinsics, ii, jj, kk, valid, jacobian, tonly):
    """transform under autograd (module docstring)"""
    if intrinsics.requires_grad:
        raise NotImplementedError("transform: the intrinsics carry no gradient (not built)")
    if tonly:
        raise NotImplementedError("transform(tonly=True) has no backward (not built)")
    _kernel_pose_rows(poses, "transform")
    if patches.dtype != torch.float32:
        raise NotImplementedError("transform: the HIP path serves float32 patches (got %s)" % patches.dtype)
    coords, mask = _TransformFn.apply(data, patches, intrinsics, ii, jj, kk, bool(valid or jacobian))
    if jacobian:
        from .lietorch import SE3
        c = patches.shape[-1] // 2
        return coords, mask[:, :, c, c], _jacobians_composed(SE3(data), patches, intrinsics, ii, jj, kk)
    return (coords, mask) if valid else coords


def transform(poses, patches, intrinsics, ii, jj, kk, depth=False, valid=False, jacobian=False, tonly=False):
    """patch k of frame i seen from frame j (projective_ops.py:53-113), one launch.

    -> coords [1,E,P,P,2]; valid=True: also (Z > 0.2) per pixel [1,E,P,P]; jacobian=True:
    (coords, (Z > 0.2) at the centre [1,E], (Ji [1,E,2,6], Jj [1,E,2,6], Jz [1,E,2,1])).  Differentiable by poses and
    patches (module docstring)."""
    if depth:
        raise NotImplementedError("transform(depth=True) is not on the update path")
    if torch.is_grad_enabled():
        data = poses if torch.is_tensor(poses) else getattr(poses, "data", None)
        if (torch.is_tensor(data) and data.requires_grad) or patches.requires_grad:
            return _transform_grad(poses, data, patches, intrinsics, ii, jj, kk, valid, jacobian, tonly)
    if not (valid or jacobian or tonly) and ops._fast and ops._env("CDV_DROPIN_FAST", "1") != "0":
        # the compiled lane (csrc/dropin_fast.cpp): the same checks, allocation and launch as below without the Python around them
        group = not torch.is_tensor(poses)
        data = getattr(poses, "data", None) if group else poses
        if torch.is_tensor(data) and data.is_cuda and not (group and getattr(poses, "group_id", None) != 3):
            r = ops._fast.transform(data, patches, intrinsics, ii, jj, kk, ops._stream())
            if r is not None:
                if type(r) is int:
                    ops._lib.check(r, "cdv_transform")
                return r.permute(0, 1, 3, 4, 2)
    if not (valid or jacobian):
        # every inference caller turns the result into [1,E,2,P,P] at once (`.permute(0, 1, 4, 2, 3).contiguous()`,
        # slam.py:328-329, loop_closure/long_term.py:118-129): the kernel writes THAT layout and the [1,E,P,P,2] tensor handed
        # back is a permuted view of it -- same values, same shape, and the caller's permute + contiguous() is then the
        # buffer itself instead of a 3.4 MB copy kernel
        return ops.transform(_kernel_pose_rows(poses, "transform"), patches, intrinsics, ii, jj, kk, layout_e2pp=True,
                             tonly=tonly).permute(0, 1, 3, 4, 2)
    return ops.transform(_kernel_pose_rows(poses, "transform"), patches, intrinsics, ii, jj, kk, layout_e2pp=False,
                         valid=valid, jacobian=jacobian, tonly=tonly)


def reproject(poses, patches, intrinsics, ii, jj, kk):
    """SLAM.reproject (cdvslam/slam.py:325-329): the coords in the [1,E,2,P,P] layout the correlation reads, written
    directly in that layout"""
    return ops.transform(_kernel_pose_rows(poses, "reproject"), patches, intrinsics, ii, jj, kk, layout_e2pp=True)


def point_cloud(poses, patches, intrinsics, ix):
    """world points of patches [1,m,3,P,P] whose frames are ix [m] -> [1,m,P,P,4] (projective_ops.py:115-117)"""
    if patches.dtype != torch.float32 or patches.shape[1] != ix.numel():
        raise NotImplementedError("point_cloud: float32 patches, one frame index per patch")
    return ops.point_cloud(_kernel_pose_rows(poses, "point_cloud"), patches, intrinsics, ix)


def flow_mag(poses, patches, intrinsics, ii, jj, kk, beta=0.3):
    """keyframe-test flow magnitude, beta * |full flow| + (1 - beta) * |translation-only flow|, and the validity mask
    (projective_ops.py:120-130) -> ([1,E,P,P] f32, [1,E,P,P] bool)"""
    if patches.dtype != torch.float32:
        raise NotImplementedError("flow_mag: float32 patches")
    return ops.flow_mag(_kernel_pose_rows(poses, "flow_mag"), patches, intrinsics, ii, jj, kk, beta)
