"""``GaussianModel`` for the render path: the parameter container PEGASUS composes scenes with
(/root/reference/src/gs/gaussian_model.py).  Same attribute names, getters (activations), PLY layout,
``merge_gaussians`` / ``mask_points`` and pose methods, and the training half: optimizer set-up (FusedAdam, one
pgr_adam_step launch per step), learning-rate schedule, densification statistics, clone / split / prune with the
optimizer state kept in step, and capture / restore for checkpoints (reference :71-104,165-191,226-229,290-458).

The pose methods run on the device: ``apply_transformation`` is one pgr_compose_object launch instead of the
reference's GPU -> CPU -> scipy/e3nn -> GPU round trip (gaussian_model.py:499-546)."""
from __future__ import annotations

import copy

import numpy as np
import torch
from torch import nn

from . import compose, pose_queue
from .ply_io import read_ply_vertices, write_ply_vertices


def strip_symmetric(L):
    return torch.stack([L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]], dim=1)


def build_rotation(r):
    q = r / torch.norm(r, dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros((q.size(0), 3, 3), device=r.device, dtype=r.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def build_scaling_rotation(s, r):
    L = torch.zeros((s.shape[0], 3, 3), dtype=s.dtype, device=s.device)
    L[:, 0, 0], L[:, 1, 1], L[:, 2, 2] = s[:, 0], s[:, 1], s[:, 2]
    return build_rotation(r) @ L


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def _posed_attribute(name):
    """_xyz / _rotation / _features_rest: what the pose calls change.  Reading or writing one applies the recorded pose
    calls first (pegasus_amd/pose_queue.py); the tensor itself lives in the instance dictionary under the same name."""
    def get(self):
        d = self.__dict__
        if d.get("_pose_ops"):
            pose_queue.flush_all()
        try:
            return d[name]
        except KeyError:
            raise AttributeError(name) from None

    def put(self, value):
        d = self.__dict__
        if d.get("_pose_ops"):
            pose_queue.flush_all()
        d[name] = value
    return property(get, put)


class GaussianModel:
    _xyz = _posed_attribute("_xyz")
    _rotation = _posed_attribute("_rotation")
    _features_rest = _posed_attribute("_features_rest")

    def __init__(self, sh_degree: int, device="cuda"):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self.device = torch.device(device)
        e = torch.empty(0)
        self._xyz = self._features_dc = self._features_rest = self._scaling = self._rotation = self._opacity = e
        self.max_radii2D = self.xyz_gradient_accum = self.denom = e
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.scaling_activation, self.scaling_inverse_activation = torch.exp, torch.log
        self.opacity_activation, self.inverse_opacity_activation = torch.sigmoid, inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize

    # ---- getters = what the rasterizer is fed (reference :105-128)
    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        L = build_scaling_rotation(scaling_modifier * self.get_scaling, self._rotation)
        return strip_symmetric(L @ L.transpose(1, 2))

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- construction
    @classmethod
    def from_arrays(cls, xyz, features_dc, features_rest, opacity, scaling, rotation, sh_degree=3, device="cuda"):
        m = cls(sh_degree, device)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(m.device).contiguous()
        m._xyz, m._features_dc, m._features_rest = t(xyz), t(features_dc), t(features_rest)
        m._opacity, m._scaling, m._rotation = t(opacity), t(scaling), t(rotation)
        m.active_sh_degree = sh_degree
        return m

    def load_ply(self, path, clean_pcd: bool = False):
        v = read_ply_vertices(path)
        if clean_pcd:
            # the reference's radius-outlier filter on the file's positions, before anything else is kept (reference :238-247)
            from .outliers import radius_outlier_mask
            pos = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32)
            v = v[radius_outlier_mask(torch.from_numpy(pos).to(self.device), 16, 0.03).cpu().numpy()]
        names = v.dtype.names
        xyz = np.stack([v["x"], v["y"], v["z"]], axis=1)
        f_dc = np.stack([v["f_dc_0"], v["f_dc_1"], v["f_dc_2"]], axis=1)[:, None, :]           # [N,1,3]
        extra = sorted((n for n in names if n.startswith("f_rest_")), key=lambda s: int(s.split("_")[-1]))
        assert len(extra) == 3 * (self.max_sh_degree + 1) ** 2 - 3
        # [N,15,3]; a degree-0 model has no f_rest_ columns at all (np.stack refuses an empty list)
        f_extra = (np.stack([v[n] for n in extra], axis=1) if extra else np.zeros((len(v), 0), np.float32)
                   ).reshape(len(v), 3, -1).transpose(0, 2, 1)
        scales = np.stack([v[n] for n in sorted((n for n in names if n.startswith("scale_")),
                                                key=lambda s: int(s.split("_")[-1]))], axis=1)
        rots = np.stack([v[n] for n in sorted((n for n in names if n.startswith("rot")),
                                              key=lambda s: int(s.split("_")[-1]))], axis=1)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float, device=self.device)
        self._xyz, self._features_dc, self._features_rest = t(xyz), t(f_dc), t(f_extra)
        self._opacity, self._scaling, self._rotation = t(np.asarray(v["opacity"])[:, None]), t(scales), t(rots)
        self.active_sh_degree = self.max_sh_degree

    def save_ply(self, path):
        c = lambda x: x.detach().cpu().numpy()
        xyz, n = c(self._xyz), self._xyz.shape[0]
        f_dc = c(self._features_dc).transpose(0, 2, 1).reshape(n, -1)
        f_rest = c(self._features_rest).transpose(0, 2, 1).reshape(n, -1)
        cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "nx": np.zeros(n), "ny": np.zeros(n), "nz": np.zeros(n)}
        cols.update({f"f_dc_{i}": f_dc[:, i] for i in range(f_dc.shape[1])})
        cols.update({f"f_rest_{i}": f_rest[:, i] for i in range(f_rest.shape[1])})
        cols["opacity"] = c(self._opacity)[:, 0]
        cols.update({f"scale_{i}": c(self._scaling)[:, i] for i in range(3)})
        cols.update({f"rot_{i}": c(self._rotation)[:, i] for i in range(4)})
        write_ply_vertices(path, cols)

    # ---- scene composition (reference :482-623)
    def _defers(self, *pose_tensors) -> bool:
        """A pose call is RECORDED (pose_queue.py) when the model lives on a HIP device, nothing of it is tracked by autograd
        and the pose arrives as a device tensor (what PEGASUS hands over); otherwise it is applied at once."""
        x = self.__dict__.get("_xyz")
        return (pose_queue.enabled() and isinstance(x, torch.Tensor) and x.is_cuda and not x.requires_grad
                and not self.__dict__["_rotation"].requires_grad and not self.__dict__["_features_rest"].requires_grad
                and all(torch.is_tensor(p) and p.is_cuda and not p.requires_grad for p in pose_tensors))

    def apply_translation_on_xyz(self, t):
        if self.__dict__.get("_pose_ops") and self._defers(t) and t.numel() == 3:
            pose_queue.record(self, pose_queue.TRANSLATE, t=pose_queue.private_copy(t))     # rides with the pending rotation
            return
        self._xyz = self._xyz + torch.as_tensor(t).to(self._xyz.device).type(torch.float32)

    def apply_rotation_on_xyz(self, R, origin=False):
        if self._defers(R) and tuple(R.shape) == (3, 3):
            pose_queue.record(self, pose_queue.ROT_XYZ, R=pose_queue.private_copy(R), origin=origin)
            return
        R = torch.as_tensor(R).to(self._xyz.device).type(torch.float32)
        if not origin:
            mean_xyz = torch.mean(self._xyz, 0)
            self._xyz = (R @ (self._xyz - mean_xyz).T).T + mean_xyz
        else:
            self._xyz = (R @ self._xyz.T).T

    def apply_transformation_on_xyz(self, T):
        if self._defers(T) and tuple(T.shape) == (4, 4):
            # ONE private copy of T; its corner and last column are addressed in place (row stride 4)
            Tc = pose_queue.private_copy(T)
            pose_queue.record(self, pose_queue.ROT_XYZ, R=Tc, R_stride=4)
            pose_queue.record(self, pose_queue.TRANSLATE, t=Tc[:3, 3], t_stride=4)
            return
        self.apply_rotation_on_xyz(R=T[:3, :3])
        self.apply_translation_on_xyz(t=T[:3, 3])

    @staticmethod
    def _host_matrix(M):
        """(key, 3x3.. float64 host copy) of a pose matrix.  PEGASUS hands the SAME device tensor R to
        apply_rotation_on_splats and apply_rotation_on_sh (pegasus_setup.py:195-208): for a tensor the key is (object,
        version counter, storage) and its host copy (one device round trip) is kept for the next call.  Host inputs
        (ndarray, lists) are COPIED and keyed on their 72 value bytes: object identity says nothing about an array the
        caller may edit in place (round-5 advisor finding)."""
        if not torch.is_tensor(M):
            host = np.array(M, dtype=np.float64, copy=True)
            return ("host", host.tobytes()), host
        try:
            key = ("tensor", id(M), M._version, M.data_ptr())
        except RuntimeError:
            key = None
        hit = GaussianModel._host_matrix_slot
        if key is not None and hit is not None and hit[0] == key:
            return key, hit[1]
        host = np.asarray(M.detach().cpu().numpy(), dtype=np.float64)
        GaussianModel._host_matrix_slot = (key, host, M)       # (keeps M alive: its id cannot be recycled under the key)
        return key, host

    _host_matrix_slot = None

    @classmethod
    def _rotation_pose(cls, R):
        """PgrObjectPose of a pure rotation about the origin (quaternion + SH band matrices), built once per R: the
        reference's update calls apply_rotation_on_splats(R) and apply_rotation_on_sh(R) with the same tensor."""
        key, host = cls._host_matrix(R)
        hit = cls._rotation_pose_slot
        if key is not None and hit is not None and hit[0] == key:
            return hit[1]
        T = np.eye(4); T[:3, :3] = host[:3, :3]
        pose = compose.make_pose(T, np.zeros(3))
        cls._rotation_pose_slot = (key, pose)
        return pose

    _rotation_pose_slot = None

    def apply_rotation_on_splats(self, R):
        """q' = q_R (x) q for every splat (reference :496-505).  Orientation only: no rotation centre is needed, so the
        object's mean is not fetched to the host (rounds 1-4 did, a device round trip per call)."""
        if self._defers(R) and tuple(R.shape) == (3, 3):
            pose_queue.record(self, pose_queue.ROT_SPLATS, R=pose_queue.private_copy(R))
            return
        out_rot = torch.empty_like(self._rotation)
        compose.compose_object(self._xyz.contiguous(), self._rotation.contiguous(), None, self._rotation_pose(R),
                               torch.empty_like(self._xyz), out_rot, None)
        self._rotation = out_rot

    def apply_rotation_on_sh(self, R):
        """SH bands 1-3 rotated with the object (reference :507-546)."""
        if self._defers(R) and tuple(R.shape) == (3, 3):
            pose_queue.record(self, pose_queue.ROT_SH, R=pose_queue.private_copy(R))
            return
        out_rest = torch.empty_like(self._features_rest)
        compose.compose_object(self._xyz.contiguous(), None, self._features_rest.contiguous(), self._rotation_pose(R),
                               torch.empty_like(self._xyz), None, out_rest)
        self._features_rest = out_rest

    def apply_transformation(self, T):
        """xyz, splat orientation and SH in ONE device pass (reference: three methods, two host round trips)."""
        if self._defers(T) and tuple(T.shape) == (4, 4):
            Tc = pose_queue.private_copy(T)
            pose_queue.record(self, pose_queue.ROT_XYZ, R=Tc, R_stride=4)
            pose_queue.record(self, pose_queue.TRANSLATE, t=Tc[:3, 3], t_stride=4)
            pose_queue.record(self, pose_queue.ROT_SPLATS, R=Tc, R_stride=4)
            pose_queue.record(self, pose_queue.ROT_SH, R=Tc, R_stride=4)
            return
        Tn = np.asarray(torch.as_tensor(T).detach().cpu().numpy(), dtype=np.float64)
        pose = compose.make_pose(Tn, self._xyz.double().mean(0).cpu().numpy())
        xyz, rot, rest = torch.empty_like(self._xyz), torch.empty_like(self._rotation), torch.empty_like(self._features_rest)
        compose.compose_object(self._xyz.contiguous(), self._rotation.contiguous(), self._features_rest.contiguous(),
                               pose, xyz, rot, rest)
        self._xyz, self._rotation, self._features_rest = xyz, rot, rest

    # The reference merges with six torch.vstack over the whole, growing scene per merged object
    # (/root/reference/src/gs/gaussian_model.py:584-591) -- 3.4 GB of copies per frame of pegasus.py:255-264 on the 2 M-Gaussian
    # scene (2.0 ms).  Here a scene that was deep-copied (what the frame loop does first) or merged into before owns row
    # buffers with spare capacity, and a merge appends the new object's rows in place: the frame's composition copies the
    # environment once and every object once.  `_rows[k] = [buffer, rows in use]`; an append is taken only if the attribute
    # still IS the leading `rows in use` rows of its buffer, so a re-assigned, masked or aliased (copy.copy) attribute falls
    # back to a fresh buffer.  Like vstack the result holds the old rows followed by the new ones; unlike vstack it shares
    # storage with the tensor it replaced.
    _ROW_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")

    @staticmethod
    def _headroom(n: int) -> int:
        return n + max(n // 2, 1 << 16)

    def _append_rows(self, k, cur, add, pending=None):
        if torch.is_grad_enabled() and (cur.requires_grad or add.requires_grad):
            return torch.vstack((cur, add))
        if cur.numel() == 0 and cur.shape[1:] != add.shape[1:]:       # a model without rows yet takes the incoming layout
            cur = add.new_empty((0,) + tuple(add.shape[1:]))
        n, m = int(cur.shape[0]), int(add.shape[0])
        rows = self.__dict__.setdefault("_rows", {})
        slot = rows.get(k)
        buf = slot[0] if slot else None
        fits = (buf is not None and slot[1] == n and n + m <= buf.shape[0] and cur.data_ptr() == buf.data_ptr() and
                cur.shape[1:] == buf.shape[1:] and cur.dtype == buf.dtype and cur.device == buf.device and cur.is_contiguous())
        if not fits:
            buf = torch.empty((self._headroom(n + m),) + tuple(cur.shape[1:]), dtype=cur.dtype, device=cur.device)
            buf[:n].copy_(cur)
        if pending is None:
            buf[n:n + m].copy_(add)
        else:
            pending.append((buf[n:n + m], add))
        rows[k] = [buf, n + m]
        return buf[:n + m]

    def merge_gaussians(self, gaussian):
        pending = []                                     # the six row copies of a merge go out as ONE multi-tensor launch
        for k in self._ROW_ATTRS:
            setattr(self, k, self._append_rows(k, getattr(self, k), getattr(gaussian, k), pending))
        if pending:
            dst, src = [d for d, _ in pending], [a for _, a in pending]
            if all(d.dtype == a.dtype and d.device == a.device for d, a in pending):
                torch._foreach_copy_(dst, src)
            else:
                for d, a in pending:
                    d.copy_(a)

    def __deepcopy__(self, memo):
        """copy.deepcopy(model): what PEGASUS's frame loop does with the environment before merging the objects into the copy
        (pegasus.py:255-256).  Same result as the default -- every tensor cloned, everything else deep-copied -- with the row
        attributes cloned into buffers that leave room for the merges that follow."""
        if self.__dict__.get("_pose_ops"):
            pose_queue.flush_all()                   # (the copy below reads the instance dictionary, not the attributes)
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        rows, dst, src = {}, [], []
        for k, v in self.__dict__.items():
            if k == "_rows":
                continue
            if (k in self._ROW_ATTRS and isinstance(v, torch.Tensor) and v.dim() >= 1 and not v.requires_grad and
                    type(v) is torch.Tensor and v.is_contiguous()):
                n = int(v.shape[0])
                buf = torch.empty((self._headroom(n),) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
                dst.append(buf[:n]); src.append(v)
                new.__dict__[k] = buf[:n]
                rows[k] = [buf, n]
            else:
                new.__dict__[k] = copy.deepcopy(v, memo)
        if dst:
            with torch.no_grad():
                if len({(t.device, t.dtype) for t in dst}) == 1:
                    torch._foreach_copy_(dst, src)            # the six row attributes in one launch
                else:
                    for d, a in zip(dst, src):
                        d.copy_(a)
        new.__dict__["_rows"] = rows
        return new

    def __copy__(self):
        """copy.copy(model): a second model over the same tensors -- never over the same list of recorded pose calls."""
        if self.__dict__.get("_pose_ops"):
            pose_queue.flush_all()
        new = self.__class__.__new__(self.__class__)
        new.__dict__.update(self.__dict__)
        return new

    def __getstate__(self):
        if self.__dict__.get("_pose_ops"):
            pose_queue.flush_all()
        return self.__dict__

    def mask_points(self, mask):
        """Keeps the rows where ``mask`` is True; with an optimizer set, in its parameters and their Adam moments too
        (reference :598-623)."""
        if self.optimizer:
            self._set_params(self._prune_optimizer(mask))
        else:
            for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
                setattr(self, k, getattr(self, k)[mask])
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            if len(getattr(self, k)) != 0:
                setattr(self, k, getattr(self, k)[mask])

    def denoise_point_cloud(self, nb_points=16, radius=0.05, debug=False):
        """Drops the Gaussians with at most ``nb_points`` positions within ``radius`` of their own, itself included
        (reference :633-651).  ``debug`` opened a viewer there; there is none here and it is ignored."""
        from .outliers import radius_outlier_mask
        self.mask_points(radius_outlier_mask(self.get_xyz.detach(), nb_points, radius))

    def translate_selected_points(self, mask, t):
        translation = torch.zeros(self._xyz.shape, device=t.device)
        translation[mask] = + t
        self._xyz = self._xyz + translation

    def create_from_pcd(self, pcd, spatial_lr_scale: float = 1.0):
        """Initial splats from a point cloud (`pcd.points` [N,3], `pcd.colors` [N,3] in 0..1), as the reference does it
        (/root/reference/src/gs/gaussian_model.py:134-162): isotropic scales from the mean distance to the three
        nearest neighbours (pegasus_amd.knn.distCUDA2), identity rotations, opacity 0.1, colours as SH degree 0."""
        from .knn import distCUDA2
        from .sh_utils import RGB2SH
        self.spatial_lr_scale = spatial_lr_scale
        dev = self.device
        pts = torch.tensor(np.asarray(pcd.points), dtype=torch.float, device=dev)
        col = RGB2SH(torch.tensor(np.asarray(pcd.colors), dtype=torch.float, device=dev))
        feats = torch.zeros((col.shape[0], 3, (self.max_sh_degree + 1) ** 2), dtype=torch.float, device=dev)
        feats[:, :3, 0] = col
        d2 = torch.clamp_min(distCUDA2(pts), 0.0000001)
        scales = torch.log(torch.sqrt(d2))[..., None].repeat(1, 3)
        rots = torch.zeros((pts.shape[0], 4), device=dev)
        rots[:, 0] = 1
        opac = torch.full((pts.shape[0], 1), 0.1, dtype=torch.float, device=dev)
        self._xyz = pts
        self._features_dc = feats[:, :, 0:1].transpose(1, 2).contiguous()
        self._features_rest = feats[:, :, 1:].transpose(1, 2).contiguous()
        self._scaling = scales
        self._rotation = rots
        self._opacity = torch.log(opac / (1 - opac))          # inverse_sigmoid
        self.max_radii2D = torch.zeros((pts.shape[0],), device=dev)

    # ---- training (reference :165-191,226-229,290-458): the optimizer holds the six row attributes as nn.Parameters;
    # every densify / prune step rebuilds them and carries their Adam moments along (new rows start at zero moments)
    _PARAM_NAMES = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
                    ("scaling", "_scaling"), ("rotation", "_rotation"))

    def _set_params(self, tensors: dict) -> None:
        for name, attr in self._PARAM_NAMES:
            if name in tensors:
                setattr(self, attr, tensors[name])

    def training_setup(self, training_args):
        from .train_ops import FusedAdam, get_expon_lr_func
        arg = lambda k, d: getattr(training_args, k, d)
        self.percent_dense = arg("percent_dense", 0.01)
        n = int(self.get_xyz.shape[0])
        dev = self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        if self.max_radii2D.shape != (n,):
            self.max_radii2D = torch.zeros((n,), device=dev)
        # the parameters get storage of their own: never a view into the row buffers of merge_gaussians / deepcopy (which a
        # later append could write) and never shared with another model
        for _, attr in self._PARAM_NAMES:
            setattr(self, attr, nn.Parameter(getattr(self, attr).detach().clone().contiguous().requires_grad_(True)))
        self.__dict__.pop("_rows", None)
        lr_init = arg("position_lr_init", 0.00016)
        feature_lr = arg("feature_lr", 0.0025)
        lrs = {"xyz": lr_init * self.spatial_lr_scale, "f_dc": feature_lr, "f_rest": feature_lr / 20.0,
               "opacity": arg("opacity_lr", 0.05), "scaling": arg("scaling_lr", 0.005), "rotation": arg("rotation_lr", 0.001)}
        groups = [{"params": [getattr(self, attr)], "lr": lrs[name], "name": name} for name, attr in self._PARAM_NAMES]
        self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=lr_init * self.spatial_lr_scale,
                                                    lr_final=arg("position_lr_final", 0.0000016) * self.spatial_lr_scale,
                                                    lr_delay_mult=arg("position_lr_delay_mult", 0.01),
                                                    max_steps=arg("position_lr_max_steps", 30_000))

    def update_learning_rate(self, iteration):
        """Position learning rate of ``iteration`` (the other groups keep theirs); returns it."""
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                lr = self.xyz_scheduler_args(iteration)
                group["lr"] = lr
                return lr

    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(),
                self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        (self.active_sh_degree, xyz, f_dc, f_rest, scaling, rotation, opacity, max_radii2D, xyz_gradient_accum, denom,
         opt_dict, self.spatial_lr_scale) = model_args
        self._xyz, self._features_dc, self._features_rest = xyz, f_dc, f_rest
        self._scaling, self._rotation, self._opacity = scaling, rotation, opacity
        self.max_radii2D = max_radii2D
        self.training_setup(training_args)
        self.xyz_gradient_accum = xyz_gradient_accum
        self.denom = denom
        self.optimizer.load_state_dict(opt_dict)

    def replace_tensor_to_optimizer(self, tensor, name):
        """Puts ``tensor`` in place of the parameter of group ``name``, with zeroed Adam moments; returns {name: param}."""
        out = {}
        for group in self.optimizer.param_groups:
            if group["name"] != name:
                continue
            old = group["params"][0]
            st = self.optimizer.state.pop(old, None)
            new = nn.Parameter(tensor.detach().contiguous().requires_grad_(True))
            group["params"][0] = new
            if st is not None:
                st["exp_avg"] = torch.zeros_like(new)
                st["exp_avg_sq"] = torch.zeros_like(new)
                self.optimizer.state[new] = st
            out[name] = new
        return out

    def _rebuild_params(self, rows_of):
        """Replaces every group's parameter p with nn.Parameter(rows_of(p, 0.0)) and its moments m with rows_of(m, 0.0):
        the one place where densification edits the optimizer."""
        out = {}
        for group in self.optimizer.param_groups:
            old = group["params"][0]
            st = self.optimizer.state.pop(old, None)
            new = nn.Parameter(rows_of(group["name"], old.detach()).contiguous().requires_grad_(True))
            group["params"][0] = new
            if st is not None:
                st["exp_avg"] = rows_of(group["name"], st["exp_avg"], moment=True).contiguous()
                st["exp_avg_sq"] = rows_of(group["name"], st["exp_avg_sq"], moment=True).contiguous()
                self.optimizer.state[new] = st
            out[group["name"]] = new
        return out

    def _prune_optimizer(self, mask):
        return self._rebuild_params(lambda name, t, moment=False: t[mask])

    def prune_points(self, mask):
        """Drops the rows where ``mask`` is True from the parameters, their Adam moments and the statistics."""
        valid = ~mask
        self._set_params(self._prune_optimizer(valid))
        self.xyz_gradient_accum = self.xyz_gradient_accum[valid]
        self.denom = self.denom[valid]
        self.max_radii2D = self.max_radii2D[valid]

    def cat_tensors_to_optimizer(self, tensors_dict):
        """Appends tensors_dict[name] to each group's parameter; the new rows start with zero Adam moments."""
        def rows_of(name, t, moment=False):
            ext = tensors_dict[name].detach()
            return torch.cat((t, torch.zeros_like(ext) if moment else ext), dim=0)
        return self._rebuild_params(rows_of)

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling,
                              new_rotation):
        self._set_params(self.cat_tensors_to_optimizer({
            "xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest, "opacity": new_opacities,
            "scaling": new_scaling, "rotation": new_rotation}))
        n, dev = int(self.get_xyz.shape[0]), self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2):
        """Gaussians with a large view-space gradient AND a large extent are replaced by N samples drawn from them, each
        with its scale divided by 0.8 N."""
        n_init = int(self.get_xyz.shape[0])
        padded = torch.zeros((n_init,), device=self._xyz.device)
        padded[:grads.shape[0]] = grads.squeeze()
        scaling = self.get_scaling
        selected = (padded >= grad_threshold) & (torch.max(scaling, dim=1).values > self.percent_dense * scene_extent)
        stds = scaling[selected].repeat(N, 1)
        samples = torch.normal(mean=torch.zeros((stds.shape[0], 3), device=stds.device), std=stds)
        rots = build_rotation(self._rotation[selected]).repeat(N, 1, 1)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self.get_xyz[selected].repeat(N, 1)
        new_scaling = self.scaling_inverse_activation(scaling[selected].repeat(N, 1) / (0.8 * N))
        self.densification_postfix(new_xyz, self._features_dc[selected].repeat(N, 1, 1),
                                   self._features_rest[selected].repeat(N, 1, 1), self._opacity[selected].repeat(N, 1),
                                   new_scaling, self._rotation[selected].repeat(N, 1))
        prune = torch.cat((selected, torch.zeros(N * int(selected.sum()), device=selected.device, dtype=torch.bool)))
        self.prune_points(prune)

    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        """Gaussians with a large view-space gradient and a small extent get an identical copy."""
        selected = (torch.norm(grads, dim=-1) >= grad_threshold) & \
                   (torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent)
        self.densification_postfix(self._xyz[selected], self._features_dc[selected], self._features_rest[selected],
                                   self._opacity[selected], self._scaling[selected], self._rotation[selected])

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        self.densify_and_clone(grads, max_grad, extent)
        self.densify_and_split(grads, max_grad, extent)
        self.prune_by(min_opacity, extent, max_screen_size)

    def prune_by(self, min_opacity, extent, max_screen_size=None):
        """Drops transparent Gaussians and, with ``max_screen_size``, those larger than it on screen (max_radii2D) or
        larger than a tenth of the scene in the world.  (Called by densify_and_prune right after densification_postfix,
        which zeroes max_radii2D, as upstream does: there only the world-size test can fire.)"""
        prune = (self.get_opacity < min_opacity).squeeze(1)
        if max_screen_size:
            big_on_screen = self.max_radii2D > max_screen_size
            big_in_world = self.get_scaling.max(dim=1).values > 0.1 * extent
            prune = prune | big_on_screen | big_in_world
        self.prune_points(prune)

    def reset_opacity(self):
        opacities_new = inverse_sigmoid(torch.min(self.get_opacity, torch.ones_like(self.get_opacity) * 0.01))
        self._opacity = self.replace_tensor_to_optimizer(opacities_new, "opacity")["opacity"]

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        """Reference form (a visibility mask): accumulates the screen-space gradient norm and the visit count."""
        g = viewspace_point_tensor.grad[update_filter, :2]
        self.xyz_gradient_accum[update_filter] += torch.norm(g, dim=-1, keepdim=True)
        self.denom[update_filter] += 1

    def add_render_stats(self, viewspace_point_tensor, radii):
        """add_densification_stats and the max_radii2D update of one render in one pgr_densify_stats launch (what the
        trainer calls: every Gaussian with radii > 0 counts)."""
        from .train_ops import densify_stats
        densify_stats(viewspace_point_tensor.grad.contiguous(), radii.to(torch.int32).contiguous(),
                      self.xyz_gradient_accum, self.denom, self.max_radii2D)

    def add_batch_render_stats(self, viewspace_point_tensor, radii, grad_scale=1.0):
        """add_render_stats for every view of a render_batch: ``viewspace_point_tensor`` [V,N,3] whose .grad holds each
        view's screen-space gradient, ``radii`` [V,N]; one pgr_densify_stats launch per view, in view order.  The gradients
        are multiplied by ``grad_scale`` first: a loss that is the MEAN of V per-view losses passes V, so that each view
        counts with its own loss's gradient and densify_grad_threshold keeps its single-view meaning."""
        from .train_ops import densify_stats
        grad = viewspace_point_tensor.grad
        radii = radii.to(torch.int32)
        for v in range(int(grad.shape[0])):
            g = grad[v] * grad_scale if grad_scale != 1.0 else grad[v]
            densify_stats(g.contiguous(), radii[v].contiguous(), self.xyz_gradient_accum, self.denom, self.max_radii2D)
