"""Host side of the rasterizer: turns torch tensors into the C-ABI structs of
include/pegasus_raster.h, manages the torch-owned workspace, and handles instance-capacity growth.

``forward_views`` renders a batch of views of one scene through ``pgr_forward``; the
drop-in ``GaussianRasterizer`` (pegasus_amd.diff_gaussian_rasterization) is the n_views == 1 case.
There is no CPU fallback anywhere in this module.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import _lib


@dataclass
class ViewSpec:
    """What GaussianRasterizationSettings says about one view (tensors stay on the device)."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    campos: torch.Tensor
    depth_mode: int = 0          # PgrDepthMode: 0 = sum T alpha z (default), 1 = normalised by 1 - T_final


class _Workspace:
    """Per-device scratch from torch's caching allocator; grown on demand, reused across calls."""

    def __init__(self):
        self.buf = {}
        self.capacity_hint = {}

    def get(self, device, nbytes: int, slot=0) -> torch.Tensor:
        key = (device, slot)
        t = self.buf.get(key)
        if t is None or t.numel() < nbytes:
            self.buf[key] = None
            del t
            t = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
            self.buf[key] = t
        return t

    def pinned(self, slot, nbytes: int) -> torch.Tensor:
        key = ("pinned", slot)
        t = self.buf.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(int(nbytes) + 64, dtype=torch.uint8).pin_memory()
            self.buf[key] = t
        return t

    def status_event(self, device, slot) -> torch.cuda.Event:
        """One event per asynchronous slot for PgrForwardCall.status_event.  torch creates the HIP event at the first
        record(); after that ``cuda_event`` is the handle the library records again on every call."""
        key = ("status-event", device, slot)
        ev = self.buf.get(key)
        if ev is None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
            self.buf[key] = ev
        return ev


_WS = _Workspace()
_LAST_INFO: dict = {}
_LAST_BLOCK_VIS = [None]     # _block_vis_words() of the call _LAST_INFO describes

MAX_INSTANCES = 0x7FFFFFFF      # per view: list positions are 32-bit (include/pegasus_raster.h)


def grown_capacity(need: int, factor: float) -> int:
    """Instance capacity for a retry after PGR_ERR_INSTANCE_OVERFLOW.  The device reports the count saturated at
    2^32 - 1; a view that needs more than MAX_INSTANCES list entries cannot be rendered and the retry gives up."""
    if need > MAX_INSTANCES:
        raise RuntimeError(f"a view lists {'>= ' if need >= 0xFFFFFFFF else ''}{need} (Gaussian, tile) instances; the "
                           f"rasterizer's per-view limit is {MAX_INSTANCES}")
    return min(MAX_INSTANCES, int(need * factor) + 1024)


def reset_capacity(hint: Optional[int] = None, *, free_workspaces: bool = True) -> None:
    """Public reset hook of the module's instance-capacity bookkeeping.

    ``hint=None`` forgets every learned capacity (the next call of each scene shape starts from its default);
    ``hint=k`` sets every capacity learned so far to ``k`` list entries per view (tests force overflows that way).
    ``free_workspaces`` also drops the cached asynchronous workspaces, so the next batch really is allocated at the new
    capacity.  The library itself keeps no state: this is host-side bookkeeping of the torch-owned scratch."""
    if hint is None:
        _WS.capacity_hint.clear()
    else:
        for key in list(_WS.capacity_hint):
            _WS.capacity_hint[key] = int(hint)
    if free_workspaces:
        drop_async_workspaces()


def drop_async_workspaces() -> None:
    """Releases the cached DEVICE workspaces of the asynchronous slots -- keys (device, ("async", slot)) -- so that the next
    batch of each slot allocates afresh.  The page-locked host scratch of a slot (("pinned", slot): a few KiB of tables and
    status words, independent of the instance capacity) stays: re-pinning memory per reset costs more than it frees."""
    for key in [k for k in _WS.buf if isinstance(k, tuple) and len(k) == 2 and isinstance(k[1], tuple) and len(k[1]) == 2
                and k[1][0] == "async"]:
        _WS.buf.pop(key)


def capacity_hints() -> dict:
    """Learned per-view instance capacities, keyed by (device, n, width, height[, "layers", n_layers])."""
    return dict(_WS.capacity_hint)


def set_capacity_hint(key, hint: Optional[int]) -> None:
    """Sets (or with ``None`` forgets) the learned capacity of one scene shape (key as in capacity_hints())."""
    if hint is None:
        _WS.capacity_hint.pop(key, None)
    else:
        _WS.capacity_hint[key] = int(hint)


def last_forward_info() -> dict:
    """Bookkeeping of the most recent forward: num_instances per view, capacities, workspace tensor."""
    return dict(_LAST_INFO)


def dev_f32(t: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    if t is None or t.numel() == 0:
        return None
    if t.device != device:
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


_ptr = _lib.ptr


def scene_struct(n: int, means3D=None, opacities=None, *, shs=None, shs_rest=None, colors_precomp=None, scales=None,
                 rotations=None, cov3D_precomp=None, sh_degree=0, scale_modifier=1.0, tie_index=None,
                 tie_inv=None) -> _lib.PgrScene:
    """The PgrScene of one call's tensors, as the kernels read them (dev_f32).  An absent tensor is a NULL pointer; the SH
    stride counts the coefficients of ``shs`` and ``shs_rest`` together, and ``tie_inv`` is passed only with ``tie_index``."""
    return _lib.PgrScene(
        n=int(n), means3d=_ptr(means3D), opacities=_ptr(opacities), scales=_ptr(scales), rotations=_ptr(rotations),
        cov3d_precomp=_ptr(cov3D_precomp), shs=_ptr(shs), colors_precomp=_ptr(colors_precomp), sh_degree=int(sh_degree),
        sh_stride=0 if shs is None else int(shs.shape[1]) + (0 if shs_rest is None else int(shs_rest.shape[1])),
        scale_modifier=float(scale_modifier), tie_index=_ptr(tie_index),
        tie_inv=None if tie_index is None else _ptr(tie_inv), shs_rest=_ptr(shs_rest))


def camera_structs(views, device):
    """The PgrCamera array of ``views`` (ViewSpecs or GaussianRasterizationSettings) and the converted camera tensors it
    points to, which must stay alive as long as the call that reads them."""
    cams = (_lib.PgrCamera * len(views))()
    keep = []
    for i, v in enumerate(views):
        bg, vm, pm, cp = (dev_f32(t, device) for t in (v.bg, v.viewmatrix, v.projmatrix, v.campos))
        keep.append((bg, vm, pm, cp))
        cams[i] = _lib.PgrCamera(image_width=int(v.image_width), image_height=int(v.image_height), tanfovx=float(v.tanfovx),
                                 tanfovy=float(v.tanfovy), viewmatrix=_ptr(vm), projmatrix=_ptr(pm), campos=_ptr(cp),
                                 bg=_ptr(bg), depth_mode=int(getattr(v, "depth_mode", 0)))
    return cams, keep


def _until_fits(run, capacity: int, factor: float, attempts: int = 3):
    """The instance-overflow retry of every forward call.  ``run(capacity)`` renders once at that per-view capacity and
    returns (status, per-view instance counts); after PGR_ERR_INSTANCE_OVERFLOW the next attempt runs at
    grown_capacity(largest count, factor).  Returns (status, counts, the capacity that held).  Raises grown_capacity's
    per-view-limit error, or RuntimeError when ``attempts`` attempts all overflowed."""
    for _attempt in range(attempts):
        status, need = run(capacity)
        if status != _lib.PGR_ERR_INSTANCE_OVERFLOW:
            return status, need, capacity
        capacity = grown_capacity(max(need), factor)
    raise RuntimeError("instance capacity did not converge")


def _learn(key, capacity: int, peak: Optional[int] = None) -> int:
    """Raises the learned capacity of ``key`` (capacity_hints()) to ``capacity``.  Given the ``peak`` count of a call that
    ran at ``capacity``, a peak above 80 % of it asks for grown_capacity(peak, 1.6) instead: few, large steps, since every
    growth reallocates the multi-GB workspace.  Returns the capacity asked for."""
    if peak is not None and peak > 0.8 * capacity:
        capacity = grown_capacity(peak, 1.6)
    _WS.capacity_hint[key] = max(_WS.capacity_hint.get(key, 0), capacity)
    return capacity


def _batch_status(scratch: torch.Tensor, nv: int):
    """(status, per-view instance counts) of the asynchronous call whose pinned host scratch is ``scratch``."""
    need = (C.c_int64 * nv)()
    status = _lib.lib().pgr_batch_status(_ptr(scratch), nv, need)
    return status, [int(x) for x in need]


def _block_vis_words(ws: torch.Tensor, n: int, width: int, height: int, capacity: int, nv: int):
    """(device pointer or None, words per block) of the visibility words a batch call of this shape, made NOW, leaves in
    ``ws`` (pgr_workspace_block_visibility: host only; None = such a call runs no block test)."""
    ptr, words = C.c_void_p(), C.c_int32()
    _lib.check(_lib.lib().pgr_workspace_block_visibility(_ptr(ws), ws.numel(), n, width, height, capacity, nv,
                                                         C.byref(ptr), C.byref(words)), "pgr_workspace_block_visibility")
    return ptr.value, int(words.value)


def _remember(key, need, used: int, ws: torch.Tensor, max_instances: Optional[int] = None, block_vis=None) -> None:
    """Fills last_forward_info() for a call of scene shape ``key`` that ran at capacity ``used`` in ``ws``; ``block_vis``:
    _block_vis_words() as asked when the call was made (None: a layered call, whose workspace is laid out differently)."""
    _LAST_INFO.clear()
    _LAST_BLOCK_VIS[0] = block_vis
    _LAST_INFO.update(num_instances=[int(x) for x in need], max_instances=int(used if max_instances is None else max_instances),
                      used_max_instances=int(used), n=int(key[1]), width=int(key[2]), height=int(key[3]),
                      n_views=len(need), workspace=ws, workspace_bytes=int(ws.numel()))


class PendingBatch:
    """Handle of an asynchronous forward_views call: ``wait()`` blocks until the batch's status words are final, checks
    the overflow flags -- after an overflow ``redo()`` renders the batch again at a grown capacity and ``redone`` is True
    -- and returns the list of result dicts.  ``keep`` holds every tensor the enqueued call reads until then."""

    def __init__(self, results, event, scratch, workspace, key, capacity, redo, keep, record_info=False, block_vis=None):
        self.results = results
        self.num_instances = None
        self.redone = False
        self._event, self._scratch, self._workspace = event, scratch, workspace
        self._key, self._capacity, self._redo, self._keep = key, capacity, redo, keep
        self._record_info = record_info      # wait() fills last_forward_info() like a synchronous call (single-view drop-in)
        self._block_vis = block_vis

    def wait(self):
        if self._event is None:
            return self.results
        self._event.synchronize()
        self._event = None
        status, self.num_instances = _batch_status(self._scratch, len(self.results))
        peak = max(self.num_instances)
        if peak > 0.8 * self._capacity:      # only a crowded batch teaches the learned capacity something
            _learn(self._key, self._capacity, peak)
        redo, self._redo = self._redo, None
        if status == _lib.PGR_ERR_INSTANCE_OVERFLOW:
            self.redone = True
            self.results = redo()
        else:
            _lib.check(status, "pgr_batch_status")
            if self._record_info:
                _remember(self._key, self.num_instances, self._capacity, self._workspace, block_vis=self._block_vis)
        return self.results


def forward_views(means3D, opacities, views: Sequence[ViewSpec], *, shs=None, colors_precomp=None, scales=None,
                  rotations=None, cov3D_precomp=None, sh_degree=0, scale_modifier=1.0, want_radii=True,
                  want_aux=False, stage_ms: Optional[list] = None, outputs: Optional[list] = None,
                  async_slot=None, semantic: Optional[dict] = None, posed: Optional[dict] = None, tie_index=None,
                  tie_inv=None, layers: Optional[dict] = None, early_status: bool = False, shs_rest=None,
                  record_info: bool = False):
    """Renders ``len(views)`` views of one scene.  Returns a list of dicts with keys
    color[3,H,W], depth[1,H,W], radii[N] (or None), and final_T / n_contrib when ``want_aux``.

    ``stage_ms``: pass an empty list to have the call timed (PgrForwardCall.stage_ms); it receives the per-stage
    milliseconds (whole batch) measured with HIP events on the launch stream.
    ``outputs``: optional pre-allocated list of dicts (same keys) to render into.
    ``async_slot``: not None -> enqueue on torch's CURRENT stream without synchronising and return a
    PendingBatch; the slot names the workspace / pinned scratch to use (one batch in flight per slot).  After an instance
    overflow its wait() renders the batch again: a layered call on the same slot, any other as the synchronous call does.
    A synchronous call with ``semantic`` or ``posed`` (and no ``stage_ms``) is an asynchronous one on the "sync-fused" slot,
    waited for; any other is a synchronous pgr_forward call on the pooled workspace.
    ``record_info`` (with ``async_slot``): PendingBatch.wait() fills last_forward_info() like a synchronous call.
    ``shs_rest``: the SH coefficients as the model stores them -- ``shs`` = _features_dc [N,1,3], ``shs_rest`` = _features_rest
    [N,K-1,3] (PgrScene::shs_rest) -- instead of their concatenation; results are bit-identical.
    ``early_status`` (with ``async_slot``, not layered): PendingBatch.wait() returns as soon as the call's status words are
    final -- behind the tile scan, PgrForwardCall.status_event -- instead of at the end of the call; the outputs are
    complete in stream order (whatever the caller queues on the current stream, or fetches with .cpu(), comes after them).
    ``semantic``: dict(object_id int32[N], colors float32[K,3], n_env, k) -> the fused objects-only semantic
    render is written to r["sem_color"] (and r["sem_depth"]) of every view (PgrForwardCall.semantic).
    ``semantic`` may also carry ``mask_colors`` float32[K,3] (+ ``mask_threshold``): every output dict with a ``sem_masks``
    uint8[K,H,W] tensor then receives the K colour-distance masks of the semantic image from the compositor's epilogue
    (bit for bit what color_masks() computes from ``sem_color``), and ``object_id_u8`` (scene_prepare()).
    An output dict with a ``record`` uint8[record_layout(H, W, K)["bytes"]] tensor (masks.record_layout; K = semantic["k"] when
    the descriptor carries mask_colors, else 0) also receives the view's frame record from the compositor's epilogue: bit
    for bit masks.pack_records of that view's color / depth / sem_masks.
    ``tie_index``: int32[N] permutation -- exact depth ties are broken by it instead of the position (PgrScene.tie_index);
    ``tie_inv``: its inverse from scene_prepare() (otherwise rebuilt per call).
    ``layers``: dict(layer_id int32[N], n_layers, mask_colors float32[n_layers,3], mask_threshold) -> LAYERED call
    (PgrForwardCall.layers, asynchronous only): Gaussian i is composited into image layer_id[i] alone and every
    output dict's ``sem_masks`` uint8[n_layers,H,W] receives the layers' masks (silhouettes); no colour image.
    ``posed``: dict(object_id int32[N], poses float32[len(views), K, 20]) -> dynamic scene: view i places object k by
    poses[i, k-1] inside the preprocess (PgrForwardCall.posed; pegasus_amd.compose.pose_table builds the rows).
    """
    L = _lib.lib()
    device = means3D.device
    if device.type != "cuda":
        raise RuntimeError("the rasterizer needs tensors on a HIP device (torch device 'cuda'); there is no CPU path")
    nv = len(views)
    if nv == 0:
        return []
    H, W = int(views[0].image_height), int(views[0].image_width)
    if any(int(v.image_height) != H or int(v.image_width) != W for v in views):
        raise ValueError("all views of a batch must share the image size")
    if posed is not None and stage_ms is not None:
        raise ValueError("a profiled call does not take posed objects")
    if layers is not None and (async_slot is None or semantic is not None or stage_ms is not None):
        raise ValueError("a layered call is asynchronous (async_slot) and takes no semantic descriptor")
    if async_slot is not None:
        stage_ms = None          # an asynchronous call is not profiled, nor is the synchronous retry of an overflow
    fused = (semantic is not None or posed is not None) and stage_ms is None
    n = int(means3D.shape[0])
    shs, shs_rest = dev_f32(shs, device), dev_f32(shs_rest, device)
    if shs_rest is not None:
        if shs is None or shs.dim() != 3 or shs.shape[1] != 1 or shs_rest.dim() != 3 or shs_rest.shape[0] != shs.shape[0]:
            raise ValueError("shs_rest goes with shs = [N,1,3] (the first coefficient) and is [N,K-1,3]")
        if shs_rest.shape[1] == 0:
            shs_rest = None                        # nothing but the first coefficient: the plain layout with stride 1
    tensors = dict(means3D=means3D, opacities=opacities, colors_precomp=colors_precomp, scales=scales, rotations=rotations,
                   cov3D_precomp=cov3D_precomp)
    tensors = {k: dev_f32(t, device) for k, t in tensors.items()}
    tensors.update(shs=shs, shs_rest=shs_rest, tie_index=tie_index, tie_inv=tie_inv)
    cams, cam_tensors = camera_structs(views, device)

    if outputs is not None:
        results = list(outputs[:nv])
    else:
        results = []
        for _ in range(nv):
            r = dict(color=torch.empty((3, H, W), dtype=torch.float32, device=device),
                     depth=torch.empty((1, H, W), dtype=torch.float32, device=device),
                     radii=torch.empty((n,), dtype=torch.int32, device=device) if want_radii else None)
            if want_aux:
                r["final_T"] = torch.empty((H, W), dtype=torch.float32, device=device)
                r["n_contrib"] = torch.empty((H, W), dtype=torch.int32, device=device)
            if semantic is not None:
                r["sem_color"] = torch.empty((3, H, W), dtype=torch.float32, device=device)
                r["sem_depth"] = torch.empty((1, H, W), dtype=torch.float32, device=device)
            results.append(r)
    outs = (_lib.PgrOutputs * nv)(*[
        _lib.PgrOutputs(color=_ptr(r.get("color")), depth=_ptr(r.get("depth")), radii=_ptr(r.get("radii")),
                        final_T=_ptr(r.get("final_T")), n_contrib=_ptr(r.get("n_contrib")),
                        sem_color=_ptr(r.get("sem_color")) if semantic is not None else None,
                        sem_depth=_ptr(r.get("sem_depth")) if semantic is not None else None,
                        sem_masks=_ptr(r.get("sem_masks")) if (semantic is not None or layers is not None) else None,
                        record=_ptr(r.get("record")) if layers is None else None)
        for r in results])

    # ONE call descriptor; an attempt sets its workspace, its capacity and what makes it synchronous or asynchronous
    call = _lib.PgrForwardCall(scene=C.pointer(scene_struct(n, sh_degree=sh_degree, scale_modifier=scale_modifier, **tensors)),
                               n_views=nv, cameras=cams, outs=outs)
    poses = None
    if posed is not None:
        poses = dev_f32(posed["poses"], device)
        if poses.dim() != 3 or poses.shape[0] != nv or poses.shape[2] != _lib.PGR_POSE_STRIDE:
            raise ValueError("posed['poses'] must be [n_views, K, 20]")
        call.posed = C.pointer(_lib.PgrPosedObjects(object_id=_ptr(posed["object_id"]), poses=_ptr(poses),
                                                    k_objects=int(poses.shape[1])))
    if semantic is not None:
        call.semantic = C.pointer(_lib.PgrSemantic(object_id=_ptr(semantic["object_id"]), colors=_ptr(semantic["colors"]),
                                                   n_env=int(semantic["n_env"]), k_objects=int(semantic["k"]),
                                                   object_id_u8=_ptr(semantic.get("object_id_u8")),
                                                   mask_colors=_ptr(semantic.get("mask_colors")),
                                                   mask_threshold=float(semantic.get("mask_threshold", 0.1))))
    key = (device, n, W, H)
    if layers is not None:
        n_layers = int(layers["n_layers"])
        call.layers = C.pointer(_lib.PgrLayers(layer_id=_ptr(layers["layer_id"]), n_layers=n_layers,
                                               mask_colors=_ptr(layers["mask_colors"]),
                                               mask_threshold=float(layers.get("mask_threshold", 0.1))))
        key += ("layers", n_layers)
    default_capacity = max(1 << 20, 6 * n)
    ws = None          # the workspace of the latest attempt
    block_vis = None   # ... and where that attempt leaves its block-visibility words (asked as the call is made)

    def workspace(slot, capacity):
        nonlocal ws, block_vis
        nbytes = (L.pgr_batch_workspace_bytes(n, W, H, capacity, nv) if layers is None else
                  L.pgr_layers_workspace_bytes(n, W, H, capacity, nv, n_layers))
        if nbytes == 0:
            raise ValueError("pgr_batch_workspace_bytes: invalid sizes")
        ws = _WS.get(device, nbytes, slot=slot)
        call.workspace, call.workspace_bytes, call.max_instances_per_view = ws.data_ptr(), ws.numel(), capacity
        block_vis = _block_vis_words(ws, n, W, H, capacity, nv) if layers is None else None

    def enqueue(slot, capacity, early=False):
        """One asynchronous attempt on ``slot``'s workspace and pinned scratch: (scratch, event behind the status words)."""
        workspace(("async", slot), capacity)
        scratch = _WS.pinned(slot, L.pgr_host_scratch_bytes(nv))
        event = _WS.status_event(device, slot) if early else torch.cuda.Event()
        call.host_scratch, call.host_scratch_bytes = scratch.data_ptr(), scratch.numel()
        call.status_event = event.cuda_event if early else None
        call.num_instances = call.stage_ms = None
        _lib.call("pgr_forward", device, call)
        if not early:
            event.record(torch.cuda.current_stream(device))
        return scratch, event

    def waited_on(slot):
        """Asynchronous attempts on ``slot``, each waited for, until the capacity holds; a grown capacity is learned."""
        def run(capacity):
            scratch, event = enqueue(slot, capacity)
            event.synchronize()
            return _batch_status(scratch, nv)
        start = _WS.capacity_hint.get(key, default_capacity)
        status, need, capacity = _until_fits(run, start, 1.6)
        _lib.check(status, "pgr_batch_status")
        if capacity != start:
            _learn(key, capacity)
        return need, capacity

    def run_plain(capacity):
        """One synchronous attempt on the pooled workspace: (status, per-view instance counts)."""
        workspace(0, capacity)
        need = (C.c_int64 * nv)()
        ms = None if stage_ms is None else (C.c_float * _lib.PGR_NUM_STAGES)()
        call.host_scratch = call.status_event = None
        call.num_instances, call.stage_ms = need, ms
        status = _lib.enqueue("pgr_forward", device, call)
        if ms is not None:
            stage_ms[:] = list(ms)
        return status, need

    def render_sync():
        if fused:
            need, capacity = waited_on("sync-fused")
            _remember(key, need, capacity, ws, block_vis=block_vis)
        else:
            status, need, capacity = _until_fits(run_plain, _WS.capacity_hint.get(key, default_capacity), 1.25)
            _lib.check(status, "pgr_forward")
            _remember(key, need, capacity, ws, max_instances=_learn(key, capacity, max(need)), block_vis=block_vis)
        return results

    def render_layers_again():       # a layered call is asynchronous only: so is its retry, on the same slot
        waited_on(async_slot)
        return results

    if async_slot is None:
        return render_sync()
    capacity = _WS.capacity_hint.get(key, default_capacity)
    scratch, event = enqueue(async_slot, capacity, early=early_status and layers is None)
    return PendingBatch(results, event, scratch, ws, key, capacity, render_sync if layers is None else render_layers_again,
                        (tensors, cam_tensors, poses, semantic, posed, layers), record_info, block_vis)


def workspace_view(view_index: int = 0) -> dict:
    """Device pointers (as ints) of view ``view_index`` inside the last forward's workspace."""
    L = _lib.lib()
    info = _LAST_INFO
    ws = info["workspace"]
    v = _lib.PgrWorkspaceView()
    _lib.check(L.pgr_workspace_view(_ptr(ws), ws.numel(), info["n"], info["width"], info["height"],
                                    info["used_max_instances"], info["n_views"], view_index, C.byref(v)),
               "pgr_workspace_view")
    return {k: getattr(v, k) for k, _ in _lib.PgrWorkspaceView._fields_}


def _unpack_visibility(words: torch.Tensor, nv: int) -> torch.Tensor:
    """int32 [groups, ceil(nv / 32)] visibility words -> bool [groups, nv]."""
    bits = (words.unsqueeze(2) >> torch.arange(32, device=words.device, dtype=torch.int32)) & 1
    return bits.reshape(words.shape[0], words.shape[1] * 32)[:, :nv].bool()


def last_block_visibility() -> Optional[torch.Tensor]:
    """bool[ceil(n / 64), n_views]: the block-visibility bits the forward call that last_forward_info() describes computed
    inside its preprocess and left in its workspace (block_visibility()'s layout and meaning), or None when that call ran
    no block test (PGR_BLOCK_CULL=0, one or two views, a small scene with its views spread over the grid).  Call it before
    the next forward on that workspace."""
    info = _LAST_INFO
    if not info:
        raise RuntimeError("last_block_visibility: no forward call on record")
    if _LAST_BLOCK_VIS[0] is None:
        raise RuntimeError("last_block_visibility: not available for a layered call")
    ptr, words = _LAST_BLOCK_VIS[0]
    if ptr is None or info["n"] == 0:
        return None
    ws = info["workspace"]
    groups = (info["n"] + 63) // 64
    off = ptr - ws.data_ptr()
    torch.cuda.current_stream(ws.device).synchronize()
    raw = ws[off:off + groups * words * 4].clone().view(torch.int32).reshape(groups, words)
    return _unpack_visibility(raw, info["n_views"])


def block_visibility(means3D, views: Sequence[ViewSpec], *, scales=None, rotations=None, cov3D_precomp=None,
                     scale_modifier=1.0) -> torch.Tensor:
    """bool[ceil(n / 64), len(views)]: False = none of the 64 Gaussians of that block can have a non-zero radius in
    that view (pgr_block_visibility: the conservative test the batch calls use internally to skip whole waves)."""
    L = _lib.lib()
    device = means3D.device
    if device.type != "cuda":
        raise RuntimeError("block_visibility needs tensors on a HIP device")
    n, nv = int(means3D.shape[0]), len(views)
    means3D, scales, rotations, cov3D_precomp = (dev_f32(t, device) for t in (means3D, scales, rotations, cov3D_precomp))
    ones = torch.ones((max(n, 1), 3), dtype=torch.float32, device=device)       # opacities / colours are not looked at
    scene = scene_struct(n, means3D, ones, colors_precomp=ones, scales=scales, rotations=rotations,
                         cov3D_precomp=cov3D_precomp, scale_modifier=scale_modifier)
    cams, _cam_tensors = camera_structs(views, device)
    groups, words = (n + 63) // 64, (nv + 31) // 32
    out = torch.zeros((groups, words), dtype=torch.int32, device=device)
    ws = torch.empty(L.pgr_block_visibility_workspace_bytes(n, nv) + 256, dtype=torch.uint8, device=device)
    _lib.call("pgr_block_visibility", device, C.byref(scene), nv, cams, _ptr(ws), ws.numel(), _ptr(out))
    torch.cuda.current_stream(device).synchronize()
    return _unpack_visibility(out, nv)


def scene_prepare(n: int, tie_index: Optional[torch.Tensor] = None, semantic: Optional[dict] = None) -> dict:
    """Per-SCENE constants of the batch calls, computed once (pgr_scene_prepare): ``tie_inv`` (inverse permutation of
    ``tie_index``) and ``object_id_u8`` (the object Gaussians' ids as bytes).  Returns a dict with those two device
    tensors (None where the input is absent) and the cache tensor that owns their memory ("cache": keep it alive)."""
    L = _lib.lib()
    ref = tie_index if tie_index is not None else (semantic["object_id"] if semantic is not None else None)
    if ref is None or n == 0:
        return dict(tie_inv=None, object_id_u8=None, cache=None)
    device = ref.device
    if device.type != "cuda":
        raise RuntimeError("scene_prepare needs tensors on a HIP device")
    scene = scene_struct(n, tie_index=tie_index)
    sem = None
    if semantic is not None:
        sem = _lib.PgrSemantic(object_id=_ptr(semantic["object_id"]), colors=_ptr(semantic["colors"]),
                               n_env=int(semantic["n_env"]), k_objects=int(semantic["k"]))
    cache = torch.empty(int(L.pgr_scene_cache_bytes(int(n))) + 256, dtype=torch.uint8, device=device)
    p_inv, p_u8 = C.c_void_p(), C.c_void_p()
    _lib.call("pgr_scene_prepare", device, C.byref(scene), C.byref(sem) if sem is not None else None, _ptr(cache),
              cache.numel(), C.byref(p_inv), C.byref(p_u8))

    def view(ptr, nbytes, dtype):
        if not ptr.value:
            return None
        off = ptr.value - cache.data_ptr()
        return cache[off:off + nbytes].view(dtype)
    n_obj = int(n) - int(semantic["n_env"]) if semantic is not None else 0
    return dict(tie_inv=view(p_inv, 4 * int(n), torch.int32), object_id_u8=view(p_u8, n_obj, torch.uint8), cache=cache)
