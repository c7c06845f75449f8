"""Drop-in for the ``diff_gaussian_rasterization`` extension PEGASUS renders through.

Same surface as the module the reference installs from its (absent) submodule
``depth-diff-gaussian-rasterization`` (/root/reference/setup.sh:19; consumers
/root/reference/src/gs/render.py:16-17,57-58,86-87,118-119 via ``gaussian_renderer.render``):

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier,
                                  viewmatrix, projmatrix, sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None,
                                        scales=None, rotations=None, cov3D_precomp=None, return_alpha=False)
        -> (color[3,H,W], radii[N] int32, depth[1,H,W])  (+ alpha[1,H,W] = 1 - final_T with return_alpha)
    GaussianRasterizer.markVisible(positions) -> bool[N]

Camera gradients: the viewmatrix, projmatrix and campos tensors of the settings are differentiable inputs too.  When
autograd is on and any of them requires grad, the render takes the differentiable path even if no scene tensor does (a
frozen model rendered from a camera being refined), and their .grad receives the exact partial of the loss with respect
to each of their entries, each treated as an independent input (PgrBackwardCall.camera_grads;
entries the forward never reads -- viewmatrix[4k+3], projmatrix[4k+2] -- get 0, campos gets 0 with colors_precomp).
A camera built from a pose (pegasus_amd.camera_pose.PosedCamera) passes them on to the pose through torch.  Without a
camera tensor that requires grad the call and its launches are those of a scene-only backward.

The compute is libpegasus_raster.so (hand-written HIP for gfx950) reached through its C ABI
(include/pegasus_raster.h); tensors are passed as raw device pointers, work is enqueued on
torch's current stream, and memory comes from torch's caching allocator.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch
from torch import nn

from .. import _lib, rasterizer
from .._lib import ptr
from ..rasterizer import _until_fits, camera_structs, dev_f32 as _dev_f32, scene_struct

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "rasterize_gaussians_batch",
           "last_forward_info", "alpha_from_final_T"]


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def last_forward_info() -> dict:
    return rasterizer.last_forward_info()


def alpha_from_final_T(final_T: torch.Tensor) -> torch.Tensor:
    """The accumulated opacity of a render, [..., 1, H, W] from the forward's final transmittance [..., H, W]."""
    return (1.0 - final_T).unsqueeze(-3)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings: GaussianRasterizationSettings, want_aux: bool = False, after_enqueue=None,
                        sh_rest=None):
    """Forward rasterization of one view.  Returns (color, radii, depth) -- plus (final_T, n_contrib)
    when ``want_aux``.

    The call is ENQUEUED without a host round trip (PgrForwardCall.status_event: tables through pinned memory), then
    ``after_enqueue(result_dict)`` runs -- work that only needs the outputs in stream order, e.g. render()'s visibility
    filter, is queued behind the compositor -- and then the host waits for the call's STATUS WORDS only, which are final
    behind the tile scan (a third into the call: the one thing the host has to decide is whether the instance capacity
    held).  The function returns while scatter, sort and compositor still run; the tensors it returns are complete in
    stream order, like the result of any torch operation.  Until round 6 it waited for the end of the call, and the GPU
    idled for the host code between two render() calls (78 us of a 0.50 ms call, profiles/r06_single_view_timeline.txt).
    ``after_enqueue`` runs again if an instance overflow re-rendered the view.
    ``sh_rest``: with it, ``sh`` is the model's _features_dc [N,1,3] and ``sh_rest`` its _features_rest [N,K-1,3]
    (PgrScene::shs_rest) -- the coefficients where they are stored, instead of get_features' concatenation."""
    rs = raster_settings
    view = rasterizer.ViewSpec(rs.image_height, rs.image_width, rs.tanfovx, rs.tanfovy, rs.bg, rs.viewmatrix,
                               rs.projmatrix, rs.campos)
    pb = rasterizer.forward_views(means3D, opacities, [view], shs=sh, colors_precomp=colors_precomp, scales=scales,
                                  rotations=rotations, cov3D_precomp=cov3Ds_precomp, sh_degree=rs.sh_degree,
                                  scale_modifier=rs.scale_modifier, want_radii=True, want_aux=want_aux,
                                  async_slot=("single-view", 0), early_status=True, shs_rest=sh_rest, record_info=True)
    if after_enqueue is not None:
        after_enqueue(pb.results[0])
    r = pb.wait()[0]
    if after_enqueue is not None and pb.redone:
        after_enqueue(r)
    if want_aux:
        return r["color"], r["radii"], r["depth"], r["final_T"], r["n_contrib"]
    return r["color"], r["radii"], r["depth"]


_SCENE_KEYS = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


class _RasterizeGaussians(torch.autograd.Function):
    """Differentiable rasterization of V views of one scene (training path): ``settings`` is a tuple of V
    GaussianRasterizationSettings with one image size.  Outputs color [V,3,H,W], radii [V,n] (not differentiable), depth
    [V,1,H,W]; gradients of the scene inputs are summed over the views, and ``means2D`` [V,n,3] receives every view's own
    screen-space gradient.  ``single`` (the drop-in GaussianRasterizer: V = 1) drops the view axis of every output and of
    ``means2D``; either way the forward is one pgr_forward call and the backward one pgr_backward call.

    The call keeps its own workspace (the backward walks the same per-tile lists), so it does not share the pooled scratch
    of the no-grad path, and retries an instance overflow with a grown capacity.  Every tensor the backward re-reads goes
    through ``ctx.save_for_backward``: an in-place update of means, scales, rotations, opacities or SH between forward and
    backward trips autograd's version-counter check instead of silently pairing new parameter values with the forward's
    lists, final_T and n_contrib.  The cameras are not re-read: the backward takes the packed ones from the workspace.

    With ``return_alpha`` a fourth output, alpha [V,1,H,W] = 1 - final_T, is differentiable: its gradient reaches the
    backward as grad_alpha (NULL when it got none).

    ``cam_inputs``: empty, or the 3 V tensors (viewmatrix, projmatrix, campos of every view, None allowed) passed when one of
    them requires grad (``_camera_inputs``).  They are the tensors ``settings`` holds, handed to ``apply`` so that autograd
    tracks them; the backward then asks for the camera gradients and returns them shaped like the tensors."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, single,
                return_alpha=False, *cam_inputs):
        L = _lib.lib()
        settings = tuple(settings)
        V = len(settings)
        if V == 0:
            raise ValueError("rasterize_gaussians_batch: no views")
        rs0 = settings[0]
        H, W = int(rs0.image_height), int(rs0.image_width)
        for rs in settings[1:]:
            if (int(rs.image_height), int(rs.image_width)) != (H, W):
                raise ValueError("rasterize_gaussians_batch: every view of a batch must have the same image size")
            if int(rs.sh_degree) != int(rs0.sh_degree) or float(rs.scale_modifier) != float(rs0.scale_modifier):
                raise ValueError("rasterize_gaussians_batch: sh_degree and scale_modifier must be the same for every view")
        device = means3D.device
        if device.type != "cuda":
            raise RuntimeError(("GaussianRasterizer" if single else "rasterize_gaussians_batch") +
                               " needs tensors on a HIP device (torch device 'cuda'); there is no CPU path")
        n = int(means3D.shape[0])
        t = {k: _dev_f32(v, device) for k, v in zip(_SCENE_KEYS, (means3D, opacities, sh, colors_precomp, scales, rotations,
                                                                  cov3Ds_precomp))}
        scene = scene_struct(n, sh_degree=rs0.sh_degree, scale_modifier=rs0.scale_modifier, **t)
        cams, _cam_tensors = camera_structs(settings, device)
        lead = () if single else (V,)
        per_view = (lambda x: (x,)) if single else (lambda x: x.unbind(0))
        color = torch.empty(lead + (3, H, W), dtype=torch.float32, device=device)
        depth = torch.empty(lead + (1, H, W), dtype=torch.float32, device=device)
        radii = torch.empty(lead + (n,), dtype=torch.int32, device=device)
        final_T = torch.empty(lead + (H, W), dtype=torch.float32, device=device)
        n_contrib = torch.empty(lead + (H, W), dtype=torch.int32, device=device)
        outs = (_lib.PgrOutputs * V)(*[
            _lib.PgrOutputs(color=ptr(c), depth=ptr(d), radii=ptr(r), final_T=ptr(ft), n_contrib=ptr(nc))
            for c, d, r, ft, nc in zip(*map(per_view, (color, depth, radii, final_T, n_contrib)))])
        need = (C.c_int64 * V)()
        ws = None
        call = _lib.PgrForwardCall(scene=C.pointer(scene), n_views=V, cameras=cams, outs=outs, num_instances=need)

        def run(capacity):
            nonlocal ws
            ws = torch.empty(L.pgr_batch_workspace_bytes(n, W, H, capacity, V), dtype=torch.uint8, device=device)
            call.workspace, call.workspace_bytes, call.max_instances_per_view = ws.data_ptr(), ws.numel(), capacity
            return _lib.enqueue("pgr_forward", device, call), need
        status, _, max_inst = _until_fits(run, max(1 << 18, 4 * n), 1.25)
        _lib.check(status, "pgr_forward")
        ctx.hw, ctx.V, ctx.n, ctx.max_inst, ctx.single = (H, W), V, n, max_inst, single
        ctx.sh_degree, ctx.scale_modifier = int(rs0.sh_degree), float(rs0.scale_modifier)
        ctx.cam_meta = tuple(None if x is None else (tuple(x.shape), x.dtype) for x in cam_inputs)
        # non-tensor state stays on ctx; tensors (inputs as the kernels read them + the forward's own buffers) are saved
        ctx.present = tuple(k for k in _SCENE_KEYS if t[k] is not None)
        ctx.op_shape = tuple(opacities.shape)
        ctx.save_for_backward(*(t[k] for k in ctx.present), ws, radii, final_T, n_contrib)
        ctx.mark_non_differentiable(radii)
        if return_alpha:
            # an output without a gradient then comes to backward as None (no zero image, no load of one)
            ctx.set_materialize_grads(False)
            return color, radii, depth, alpha_from_final_T(final_T)
        return color, radii, depth

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_depth, grad_alpha=None):
        L = _lib.lib()
        V, n, (H, W), single = ctx.V, ctx.n, ctx.hw, ctx.single
        saved = ctx.saved_tensors          # raises if an input was modified in place since the forward
        k = len(ctx.present)
        t = dict(zip(ctx.present, saved[:k]))
        ws, radii, final_T, n_contrib = saved[k:]
        device = ws.device
        lead = () if single else (V,)
        # preprocess_backward_batch_kernel writes every element of every gradient it is handed (zeros for culled
        # Gaussians): no zero fill (384 MB for the SH gradient of a 2 M-Gaussian scene) -- except for an empty scene,
        # where nothing runs
        alloc = torch.empty if n > 0 else torch.zeros
        z = lambda *shape: alloc(shape, dtype=torch.float32, device=device)
        g = dict(means2d=z(*lead, n, 3), means3d=z(n, 3), opacities=z(n, 1))
        if "shs" in t:
            g["shs"] = z(*t["shs"].shape)
        else:
            g["colors"] = z(n, 3)
        if "cov3D_precomp" in t:
            g["cov3d"] = z(n, 6)
        else:
            g["scales"], g["rotations"] = z(n, 3), z(n, 4)
        grads = _lib.PgrGradOutputs(**{key: ptr(v) for key, v in g.items()})
        scene = scene_struct(n, sh_degree=ctx.sh_degree, scale_modifier=ctx.scale_modifier, **t)
        cams = (_lib.PgrCamera * V)(*[_lib.PgrCamera(image_width=W, image_height=H) for _ in range(V)])
        gc = (torch.zeros(lead + (3, H, W), dtype=torch.float32, device=device) if grad_color is None
              else grad_color.contiguous().float())
        gd = None if grad_depth is None else grad_depth.contiguous().float()
        ga = None if grad_alpha is None else grad_alpha.contiguous().float()
        per_view = lambda x: (None,) * V if x is None else (x,) if single else x.unbind(0)
        views = (_lib.PgrBackwardView * V)(*[
            _lib.PgrBackwardView(grad_color=ptr(c), grad_depth=ptr(d), final_T=ptr(ft), n_contrib=ptr(nc), radii=ptr(r))
            for c, d, ft, nc, r in zip(*map(per_view, (gc, gd, final_T, n_contrib, radii)))])
        scratch = torch.empty(max(1, L.pgr_backward_batch_scratch_bytes(n, V)), dtype=torch.uint8, device=device)
        call = _lib.PgrBackwardCall(scene=C.pointer(scene), n_views=V, cameras=cams, views=views, workspace=ws.data_ptr(),
                                    workspace_bytes=ws.numel(), max_instances_per_view=ctx.max_inst, grads=C.pointer(grads),
                                    scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
        if ga is not None:
            call.grad_alpha = (C.c_void_p * V)(*[a.data_ptr() for a in per_view(ga)])
        # camera gradients: [V, 35] written by the camera kernels (only the wanted ones get a pointer); without them the
        # call and its launches are the scene-only ones
        want_cam = [m is not None and ctx.needs_input_grad[11 + j] for j, m in enumerate(ctx.cam_meta)]
        sl = ((0, 16), (16, 32), (32, 35))
        cam_g = None
        if any(want_cam):
            cam_g = torch.empty((V, 35), dtype=torch.float32, device=device)
            call.camera_grads = (_lib.PgrCameraGrad * V)(*[_lib.PgrCameraGrad(*[
                ptr(cam_g[v, a:b]) if want_cam[3 * v + c] else None for c, (a, b) in enumerate(sl)]) for v in range(V)])
            cam_scratch = torch.empty(L.pgr_camera_grad_scratch_bytes(n, V), dtype=torch.uint8, device=device)
            call.camera_scratch, call.camera_scratch_bytes = cam_scratch.data_ptr(), cam_scratch.numel()
        _lib.call("pgr_backward", device, call)
        cam_out = tuple(cam_g[j // 3, sl[j % 3][0]:sl[j % 3][1]].reshape(m[0]).to(m[1]) if want_cam[j] else None
                        for j, m in enumerate(ctx.cam_meta))
        # means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, single, return_alpha,
        # then the camera tensors
        return (g["means3d"], g["means2d"], g.get("shs"), g.get("colors"), g["opacities"].view(ctx.op_shape),
                g.get("scales"), g.get("rotations"), g.get("cov3d"), None, None, None) + cam_out


def _camera_inputs(settings) -> tuple:
    """The camera tensors of ``settings`` as extra ``_RasterizeGaussians`` inputs: all 3 V of them (viewmatrix, projmatrix,
    campos per view) when autograd is on and one of them requires grad, else none (the scene-only call)."""
    cams = tuple(x for rs in settings for x in (rs.viewmatrix, rs.projmatrix, rs.campos))
    if torch.is_grad_enabled() and any(isinstance(x, torch.Tensor) and x.requires_grad for x in cams):
        return tuple(x if isinstance(x, torch.Tensor) else None for x in cams)
    return ()


def rasterize_gaussians_batch(means3D, means2D, opacities, raster_settings, shs=None, colors_precomp=None, scales=None,
                              rotations=None, cov3D_precomp=None, return_alpha=False):
    """Differentiable render of V views of one scene: ``raster_settings`` is a sequence of V
    GaussianRasterizationSettings with one image size.  Returns (color [V,3,H,W], radii [V,n] int32, depth [V,1,H,W]), and
    with ``return_alpha`` also alpha [V,1,H,W] = 1 - final_T (differentiable).
    ``means2D`` (or None) is [V,n,3]; its .grad receives each view's screen-space gradient.  Every other input's gradient
    is the sum over the views.  A view's viewmatrix / projmatrix / campos that requires grad receives that view's camera
    gradient."""
    if (shs is None) == (colors_precomp is None):
        raise ValueError("rasterize_gaussians_batch: provide exactly one of shs and colors_precomp")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise ValueError("rasterize_gaussians_batch: provide exactly one of a scale/rotation pair and cov3D_precomp")
    settings = tuple(raster_settings)
    if means2D is None:
        means2D = torch.zeros((len(settings), int(means3D.shape[0]), 3), dtype=torch.float32, device=means3D.device)
    return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                     settings, False, bool(return_alpha), *_camera_inputs(settings))


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """bool[N]: Gaussian centre is in front of the near plane of this view."""
        with torch.no_grad():
            device = positions.device
            if device.type != "cuda":
                raise RuntimeError("markVisible needs a HIP device tensor")
            pos = _dev_f32(positions, device)
            n = int(positions.shape[0])
            present = torch.zeros((n,), dtype=torch.uint8, device=device)
            if n:
                view = _dev_f32(self.raster_settings.viewmatrix, device)
                _lib.call("pgr_mark_visible", device, n, ptr(pos), ptr(view), ptr(present))
            return present.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, return_alpha=False):
        """(color, radii, depth), or (color, radii, depth, alpha) with ``return_alpha``: alpha [1,H,W] = 1 - final_T, the
        accumulated opacity, differentiable like the colour."""
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        inputs = (means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp)
        cams = _camera_inputs((self.raster_settings,))
        if cams or (torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in inputs)):
            if means2D is None:
                means2D = torch.zeros_like(means3D, requires_grad=False)
            return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                             cov3D_precomp, (self.raster_settings,), True, bool(return_alpha), *cams)
        with torch.no_grad():
            if return_alpha:
                color, radii, depth, final_T, _ = rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities,
                                                                      scales, rotations, cov3D_precomp,
                                                                      self.raster_settings, want_aux=True)
                return color, radii, depth, alpha_from_final_T(final_T)
            return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                       cov3D_precomp, self.raster_settings)
