"""ctypes binding of ``libk2b.so`` (C ABI: ``include/k2b.h``).

PyTorch is used here only for device memory and streams.  There is no CPU
fallback: if the library is missing, or no HIP device is visible, every entry
point raises ``RuntimeError`` (the product path must fail loudly).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

_LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libk2b.so"
_lib = None

K2B_OK = 0
K2B_ERR_INVALID_ARGUMENT = -1
K2B_ERR_UNSUPPORTED = -2
K2B_ERR_HIP = -3
K2B_ERR_NO_DEVICE = -4

class FitConfigC(C.Structure):
    """Mirror of ``k2b_fit_config`` (include/k2b.h)."""

    _fields_ = [
        ("num_iters", C.c_int32),
        ("step_size", C.c_double),
        ("adam_beta1", C.c_double),
        ("adam_beta2", C.c_double),
        ("adam_eps", C.c_double),
        ("sigma", C.c_float),
        ("joint_loss_weight", C.c_float),
        ("pose_prior_weight", C.c_float),
        ("angle_prior_weight", C.c_float),
        ("shape_prior_weight", C.c_float),
        ("pose_preserve_weight", C.c_float),
        ("freeze_betas", C.c_int32),
        ("conf_per_frame", C.c_int32),
        ("angle_prior_index", C.c_int32 * 4),
        ("angle_prior_sign", C.c_float * 4),
        ("optimize_mask", C.c_int32),
        ("transl_prior_weight", C.c_float),
        ("debug_launch_shape", C.c_int32),
        ("prior_pose_dims", C.c_int32),
        ("num_betas_prior", C.c_int32),
        ("projection", C.c_int32),
        ("focal", C.c_float * 2),
    ]


class CameraC(C.Structure):
    """Mirror of ``k2b_camera`` (include/k2b.h): row-major world-to-camera rotation, translation, focals in pixels."""

    _fields_ = [("rotation", C.c_float * 9), ("translation", C.c_float * 3), ("focal", C.c_float * 2)]


def library_path() -> Path:
    return _LIB_PATH


_vp, _i32, _i64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
_FIT_HEAD = (_vp, _vp, C.POINTER(FitConfigC))       # model, prior, cfg
_FIT_IN = (_i32, _vp) + (_vp,) * 6                  # num_targets, model_joint_index, j3d, conf, the four start parameters
_FIT_OUT = (_vp,) * 5                               # the four fitted parameters, loss
_LBFGS_TAIL = (_i32, _f64, _f64, _f64)              # history_size, lr, tolerance_grad, tolerance_change
_STREAM = (_vp,)

# (symbol, restype, argtypes) of every declaration of include/k2b.h; tests/test_host_logic.py holds the two together
_PROTOTYPES = (
    ("k2b_version", C.c_uint32, ()),
    ("k2b_last_error", C.c_char_p, ()),
    ("k2b_model_create", C.c_int, (C.POINTER(_vp),) + (_i32,) * 4 + (_vp,) * 7),
    ("k2b_model_destroy", None, (_vp,)),
    ("k2b_model_dims", C.c_int, (_vp,) + (C.POINTER(_i32),) * 4),
    ("k2b_model_joint_basis", C.c_int, (_vp, _vp, _vp)),
    ("k2b_model_reserve", C.c_int, (_vp, _i32)),
    ("k2b_debug_read_dump", C.c_int, (_vp, _vp, _i64)),
    ("k2b_prior_create", C.c_int, (C.POINTER(_vp), _i32, _i32, _vp, _vp, _vp)),
    ("k2b_prior_destroy", None, (_vp,)),
    ("k2b_fit_config_default", None, (C.POINTER(FitConfigC),)),
    ("k2b_fit_config_size", C.c_uint32, ()),
    ("k2b_fit_world", C.c_int, _FIT_HEAD + (_i32,) + _FIT_IN + (_vp, _vp) + _FIT_OUT + (_vp,) + _STREAM),
    ("k2b_fit_sequence", C.c_int, _FIT_HEAD + (_i32, _i32, _i32) + _FIT_IN + _FIT_OUT + _STREAM),
    ("k2b_lbs", C.c_int, (_vp, _i32) + (_vp,) * 6 + _STREAM),
    ("k2b_vertex_term", C.c_int, (_vp, _i32, _i32, _vp, _vp, _vp, _f32, _f32) + (_vp,) * 6 + _STREAM),
    ("k2b_adam_step", C.c_int, (_i64,) + (_vp,) * 4 + (_i32,) + (_f64,) * 4 + _STREAM),
    ("k2b_angular_error_deg", C.c_int, (_i64, _vp, _vp, _vp) + _STREAM),
    ("k2b_fit_world_lbfgs", C.c_int,
     _FIT_HEAD + (_i32,) + _FIT_IN + (_vp, _vp) + _FIT_OUT + (_vp,) + (_i32,) + _LBFGS_TAIL + _STREAM),
    ("k2b_fit_sequence_lbfgs", C.c_int, _FIT_HEAD + (_i32,) + _FIT_IN + _FIT_OUT + (_i32, _i32) + _LBFGS_TAIL + _STREAM),
    ("k2b_model_set_landmarks", C.c_int, (_vp, _i32, _vp, _vp)),
    ("k2b_model_num_landmarks", C.c_int, (_vp, C.POINTER(_i32))),
    ("k2b_surface_term", C.c_int, (_vp, _i32, _i32, _vp, _vp, _vp, _i32, _f32, _f32) + (_vp,) * 6 + _STREAM),
    ("k2b_ikgat_create", C.c_int, (C.POINTER(_vp),) + (_i32,) * 5 + (_vp, _vp, _i64)),
    ("k2b_ikgat_destroy", None, (_vp,)),
    ("k2b_ikgat_predict", C.c_int, (_vp, _i32, _vp, _vp, _i32, _vp) + _STREAM),
    ("k2b_fit_sequences", C.c_int, _FIT_HEAD + (_i32, _vp, _vp, _i32) + _FIT_IN + _FIT_OUT + _STREAM),
    ("k2b_fit_sequences_lbfgs", C.c_int,
     _FIT_HEAD + (_i32, _vp, _vp) + _FIT_IN + _FIT_OUT + (_i32, _i32) + _LBFGS_TAIL + _STREAM),
    ("k2b_sequence_order", C.c_int, (_i32, _vp, _vp, _vp, C.POINTER(_i32))),
    ("k2b_shape_pass_lbfgs", C.c_int,
     _FIT_HEAD + (_i32, _vp, _i32, _i32, _vp) + (_vp,) * 5 + (_i32, _i32, _vp, _vp, _i32) + _LBFGS_TAIL + _STREAM),
    ("k2b_lbs_backward", C.c_int, (_vp, _i32) + (_vp,) * 10 + _STREAM),
    ("k2b_debug_lbfgs_state_layout", C.c_int, (_i32, _i32, _i32) + (C.POINTER(_i64),) * 3 + (C.POINTER(_i32),) * 2),
    ("k2b_debug_lbfgs_step", C.c_int, (_i32, _i32, _i32) + (_vp,) * 6 + (_i32, _i32, _f64, _f64, _f64, _vp, _i64, _i32, _i32) + _STREAM),
    ("k2b_point_error", C.c_int, (_i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp) + _STREAM),
    ("k2b_fit_image_sequences", C.c_int, _FIT_HEAD + (_i32, _vp, _vp, _i32, _i32) + _FIT_IN + _FIT_OUT + _STREAM),
    ("k2b_fit_image", C.c_int, _FIT_HEAD + (_i32,) + _FIT_IN + (_vp, _vp) + _FIT_OUT + (_vp,) + _STREAM),
    ("k2b_surface_term_image", C.c_int, (_vp, _i32, _i32, _vp, _vp, _vp, _i32, _f32, _f32, _vp) + (_vp,) * 6 + _STREAM),
    ("k2b_camera_size", C.c_uint32, ()),
    ("k2b_fit_multiview", C.c_int, _FIT_HEAD + (_i32, _i32, C.POINTER(CameraC)) + _FIT_IN + (_vp, _vp) + _FIT_OUT + (_vp,) + _STREAM),
    ("k2b_fit_multiview_sequences", C.c_int,
     _FIT_HEAD + (_i32, _vp, _vp, _i32, _i32, _i32, C.POINTER(CameraC)) + _FIT_IN + _FIT_OUT + _STREAM),
)
EXPORTED_SYMBOLS = tuple(name for name, _, _ in _PROTOTYPES)


def load_library():
    """dlopen ``libk2b.so`` and declare prototypes (no device call is made)."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise RuntimeError(
            f"{_LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C keypoints2body_amd/csrc). "
            "keypoints2body_amd has no CPU fallback."
        )
    lib = C.CDLL(str(_LIB_PATH))
    for name, restype, argtypes in _PROTOTYPES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
        if name == "k2b_fit_config_size" and fn() != C.sizeof(FitConfigC):     # before any prototype that takes the struct is used
            raise RuntimeError("libk2b.so was built with a different k2b_fit_config layout than native.FitConfigC")
        if name == "k2b_camera_size" and fn() != C.sizeof(CameraC):
            raise RuntimeError("libk2b.so was built with a different k2b_camera layout than native.CameraC")
    _lib = lib
    return lib


def _check(code: int, what: str):
    if code == K2B_OK:
        return
    msg = load_library().k2b_last_error().decode("utf-8", "replace")
    text = f"{what}: {msg}"
    if code == K2B_ERR_INVALID_ARGUMENT:
        raise ValueError(text)
    if code == K2B_ERR_UNSUPPORTED:
        raise NotImplementedError(text)
    raise RuntimeError(text)


def _host_f32(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _host_i32(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.int32)


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _dev(t: Optional[torch.Tensor], name: str, device: torch.device, shape=None):
    """Validated device pointer of a contiguous float32 tensor (None -> NULL)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 torch tensor")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return C.c_void_p(t.data_ptr())


# ---- the one place a result is allocated ---------------------------------------------------------------------------------------------
class _Outputs(threading.local):
    provider = None                   # the innermost ``outputs_from`` of this thread (the class default: none; a plain attribute read)


_outputs = _Outputs()


@contextlib.contextmanager
def outputs_from(provider):
    """Inside the block every wrapper of this module asks ``provider(name, shape)`` for each result tensor before it allocates
    one: a tensor is used as that result (validated as an input is: device, float32, contiguous, exact shape), ``None`` means
    "allocate as before".  So a caller can pass the output buffers of the C ABI: its own arena, or - for the four fitted
    parameters of ``fit_world`` / ``fit_image`` / ``fit_multiview`` / ``fit_world_lbfgs`` - the input tensors themselves (k2b.h,
    Conventions: aliasing).  Per thread, nestable (the innermost provider is asked, and it alone), restored on exit and on
    exceptions; ``outputs_from(None)`` switches an outer provider off.

    `name` is the key of the result: ``global_orient``, ``body_pose``, ``betas``, ``transl``, ``loss``, ``grad`` (the fit entries, in
    this order; ``shape_pass_lbfgs``: ``betas``; the stand-alone terms: ``loss``, ``grad``), ``joints``, ``vertices``
    (``NativeModel.lbs``), ``grad_global_orient``, ``grad_body_pose``, ``grad_betas``, ``grad_transl`` (``lbs_backward``), ``deg``
    (``angular_error_deg``), ``err``, ``per_point``, ``transform`` (``point_error``), ``quaternions`` (``NativeIkgat.predict``).
    ``adam_step`` works in place and asks for nothing."""
    before = _outputs.provider
    _outputs.provider = provider
    try:
        yield
    finally:
        _outputs.provider = before


def _output(name: str, shape, device: torch.device) -> torch.Tensor:
    """The result tensor `name` of a call: the current provider's (``outputs_from``), else a fresh ``torch.empty``."""
    provider = _outputs.provider                                  # the whole cost outside ``outputs_from``: one thread-local read
    if provider is not None:
        shape = tuple(int(n) for n in shape)
        given = provider(name, shape)
        if given is not None:
            _dev(given, f"the provided output {name}", device, shape)
            return given
    return torch.empty(shape, dtype=torch.float32, device=device)


def require_device(device=None) -> torch.device:
    """Resolve a HIP device or raise: the engine has no CPU path."""
    if not torch.cuda.is_available():
        raise RuntimeError("keypoints2body_amd needs a HIP device (MI355X / gfx950); none is visible and there is no CPU fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError(f"keypoints2body_amd runs on HIP devices only, got device={dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class _Handle:
    """Owner of one library handle in ``_h``; ``_destroy`` names the symbol that frees it when the owner goes."""

    _destroy = ""

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value and _lib is not None:
                getattr(_lib, self._destroy)(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


def _launch(name: str, dev: torch.device, *args):
    """The one way into a stream-ordered entry: on `dev`, ``<name>(*args, current stream)``, a failure status raised.
    (``getattr`` on the CDLL is the attribute read ``lib.<name>`` is: ctypes caches the function on first use.)"""
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(getattr(load_library(), name)(*args, stream), name)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class NativeModel(_Handle):
    """Owner of a ``k2b_model`` handle (body-model constants in HBM)."""

    _destroy = "k2b_model_destroy"

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, lbs_weights, parents,
                 extra_vertex_ids, device=None, landmarks=None):
        """`landmarks`: optional ``(vertex_ids [L,3] int, bary [L,3] float)``, smplx's facial landmarks
        (``faces_tensor[lmk_faces_idx]``, ``lmk_bary_coords``): output joints J+E .. J+E+L-1."""
        self.device = require_device(device)
        lib = load_library()
        vt = _host_f32(v_template)
        sd = _host_f32(shapedirs)
        pd = _host_f32(posedirs)
        jr = _host_f32(J_regressor)
        lw = _host_f32(lbs_weights)
        par = _host_i32(parents).copy()
        par[0] = -1      # smplx stores the root's parent as a huge unsigned sentinel
        ex = _host_i32(extra_vertex_ids if extra_vertex_ids is not None else np.zeros(0, np.int32))
        V, J, NB, E = vt.shape[0], par.shape[0], sd.shape[2], ex.shape[0]
        if vt.shape != (V, 3) or sd.shape != (V, 3, NB) or pd.shape != (9 * (J - 1), 3 * V) \
                or jr.shape != (J, V) or lw.shape != (V, J):
            raise ValueError(
                f"inconsistent body-model constants: v_template {vt.shape}, shapedirs {sd.shape}, posedirs {pd.shape}, "
                f"J_regressor {jr.shape}, lbs_weights {lw.shape}, parents {par.shape}")
        lm_ids = lm_w = None
        if landmarks is not None:
            lm_ids, lm_w = _host_i32(landmarks[0]), _host_f32(landmarks[1])
            if lm_ids.ndim != 2 or lm_ids.shape[1] != 3 or lm_w.shape != lm_ids.shape:
                raise ValueError(f"landmarks must be (vertex_ids [L,3], bary [L,3]), got {lm_ids.shape} and {lm_w.shape}")
        self.num_vertices, self.num_joints, self.num_betas, self.num_extra = V, J, NB, E
        self.num_landmarks = 0
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(lib.k2b_model_create(C.byref(self._h), V, J, NB, E, _np_ptr(vt), _np_ptr(sd), _np_ptr(pd),
                                        _np_ptr(jr), _np_ptr(lw), _np_ptr(par), _np_ptr(ex)), "k2b_model_create")
            if lm_ids is not None:
                _check(lib.k2b_model_set_landmarks(self._h, lm_ids.shape[0], _np_ptr(lm_ids), _np_ptr(lm_w)),
                       "k2b_model_set_landmarks")
                n = C.c_int32(0)
                _check(lib.k2b_model_num_landmarks(self._h, C.byref(n)), "k2b_model_num_landmarks")
                self.num_landmarks = int(n.value)

    @property
    def num_output_joints(self) -> int:
        """Rows of ``lbs``'s joints: J kinematic, E vertex-selected, L landmarks (smplx's layout)."""
        return self.num_joints + self.num_extra + self.num_landmarks

    @property
    def handle(self):
        return self._h

    def reserve(self, max_frames: int) -> None:
        """Pre-size the LBS workspace: no later ``lbs`` call of up to `max_frames` frames allocates or synchronises."""
        with torch.cuda.device(self.device):
            _check(load_library().k2b_model_reserve(self._h, int(max_frames)), "k2b_model_reserve")

    def joint_basis(self):
        jt = np.zeros((self.num_joints, 3), np.float32)
        jd = np.zeros((self.num_joints, 3, self.num_betas), np.float32)
        _check(load_library().k2b_model_joint_basis(self._h, _np_ptr(jt), _np_ptr(jd)), "k2b_model_joint_basis")
        return jt, jd

    def lbs(self, global_orient, body_pose, betas, transl=None, want_vertices=True):
        """Full forward: returns (joints (B,J+E+L,3), vertices (B,V,3) or None)."""
        dev = self.device
        B = global_orient.shape[0]
        params = _param_ptrs(self, B, global_orient, body_pose, betas, transl)
        joints = _output("joints", (B, self.num_output_joints, 3), dev)
        verts = _output("vertices", (B, self.num_vertices, 3), dev) if want_vertices else None
        _launch("k2b_lbs", dev, self._h, B, *params, _ptr(joints), _ptr(verts))
        return joints, verts

    def dev_read_x(self, halfs: int):
        """Development entry ``k2b_dev_lbs_read_x`` (outside include/k2b.h): the first `halfs` halfs of the X workspace, hi and lo
        pieces as two uint16 arrays, as the last ``lbs`` call left them.  Synchronises the device."""
        fn = load_library().k2b_dev_lbs_read_x
        fn.restype, fn.argtypes = C.c_int, [_vp, _vp, _vp, _i64]
        xh, xl = np.empty(int(halfs), dtype=np.uint16), np.empty(int(halfs), dtype=np.uint16)
        with torch.cuda.device(self.device):
            if fn(self._h, _np_ptr(xh), _np_ptr(xl), int(halfs)) != 0:
                raise ValueError(f"k2b_dev_lbs_read_x: {halfs} halfs refused (NULL argument, size above the workspace, or a HIP error)")
        return xh, xl

    def lbs_backward(self, global_orient, body_pose, betas, transl, grad_joints, grad_vertices, want=(True, True, True, True)):
        """Vector-Jacobian product of ``lbs``: the gradients of (global_orient, body_pose, betas, transl) for the cotangents
        `grad_joints` (B,J+E+L,3) and / or `grad_vertices` (B,V,3) (either may be None, not both); an entry of `want` that is
        false leaves its gradient out (None in the result).  ``transl`` may be None; its gradient is defined all the same."""
        dev = self.device
        B = global_orient.shape[0]
        params = _param_ptrs(self, B, global_orient, body_pose, betas, transl)
        gj = _dev(grad_joints, "grad_joints", dev, (B, self.num_output_joints, 3))
        gv = _dev(grad_vertices, "grad_vertices", dev, (B, self.num_vertices, 3))
        grads = [_output(f"grad_{k}", (B, w), dev) if wanted else None
                 for k, w, wanted in zip(PARAM_KEYS, _param_widths(self), want)]
        _launch("k2b_lbs_backward", dev, self._h, B, *params, gj, gv, *(_ptr(g) for g in grads))
        return tuple(grads)


class NativePrior(_Handle):
    """Owner of a ``k2b_prior`` handle built from the reference prior's buffers."""

    _destroy = "k2b_prior_destroy"

    def __init__(self, means, precisions, nll_weights, device=None):
        self.device = require_device(device)
        mu = _host_f32(means)
        pr = _host_f32(precisions)
        nw = _host_f32(nll_weights).reshape(-1)
        M, D = mu.shape
        if pr.shape != (M, D, D) or nw.shape != (M,):
            raise ValueError(f"prior buffers disagree: means {mu.shape}, precisions {pr.shape}, nll_weights {nw.shape}")
        self.num_gaussians, self.dim = M, D
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(load_library().k2b_prior_create(C.byref(self._h), M, D, _np_ptr(mu), _np_ptr(pr), _np_ptr(nw)),
                   "k2b_prior_create")

    @property
    def handle(self):
        return self._h


def default_fit_config() -> FitConfigC:
    cfg = FitConfigC()
    load_library().k2b_fit_config_default(C.byref(cfg))
    return cfg


# ---- the one description of a fit call -----------------------------------------------------------------------------
PARAM_KEYS = ("global_orient", "body_pose", "betas", "transl")   # order of the packed parameter / gradient row (k2b.h, grad_out)


def param_columns(D: int, NB: int) -> dict:
    """Column slices of the packed row ``[global_orient | body_pose | betas | transl]`` for a pose of `D` = 3 (J - 1) values and
    `NB` shape coefficients: the layout of ``grad`` and of the host-driven L-BFGS twins' parameter rows."""
    edges = (0, 3, 3 + D, 3 + D + NB, 3 + D + NB + 3)
    return {k: slice(a, b) for k, a, b in zip(PARAM_KEYS, edges, edges[1:])}


def _param_widths(model: NativeModel):
    return 3, 3 * (model.num_joints - 1), model.num_betas, 3


def _param_ptrs(model: NativeModel, rows: int, global_orient, body_pose, betas, transl):
    """Validated pointers of `rows` rows of parameters."""
    return [_dev(t, k, model.device, (rows, w))
            for k, w, t in zip(PARAM_KEYS, _param_widths(model), (global_orient, body_pose, betas, transl))]


def _joint_index(index, count: int, name: str = "model_joint_index") -> np.ndarray:
    """Host int32 joint per target, one entry per target."""
    idx = _host_i32(np.asarray(list(index)))
    if idx.shape != (count,):
        raise ValueError(f"{name} has {idx.shape[0]} entries for {count} targets")
    return idx


def _fit_outputs(model: NativeModel, lead: tuple, want_grad: bool = False) -> dict:
    """The result tensors of a fit over frames of leading shape `lead` (+ ``grad`` in the packed layout)."""
    new = lambda name, *shape: _output(name, lead + shape, model.device)
    widths = _param_widths(model)
    out = {k: new(k, w) for k, w in zip(PARAM_KEYS, widths)}
    out["loss"] = new("loss")
    if want_grad:
        out["grad"] = new("grad", sum(widths))
    return out


def _lbfgs_tail(history_size, lr, tolerance_grad, tolerance_change):
    return int(history_size), float(lr), float(tolerance_grad), float(tolerance_change)


def _fit_call(name: str, model: NativeModel, prior: NativePrior, cfg: FitConfigC, head: tuple, idx: np.ndarray, lead: tuple,
              starts: int, j3d, conf, global_orient, body_pose, betas, transl, tail: tuple = (), world: Optional[tuple] = None,
              out_lead: Optional[tuple] = None):
    """Set-up and launch of every fit entry.  The C arguments are (model, prior, cfg, *`head`, K, joint index, targets of
    leading shape `lead`, confidences, `starts` rows of start parameters, [preserve_pose, transl_prior_target], the five
    outputs, [grad], *`tail`, stream); the bracketed ones belong to ``k2b_fit_world*`` and come with
    `world` = (preserve_pose, transl_prior_target, want_grad).  `out_lead`: the leading shape of the outputs where it is not
    `lead` (several views: targets (B, C, K, 3), shared confidences (C, K), outputs (B, .))."""
    dev, K = model.device, idx.shape[0]
    conf_p = _dev(conf, "conf", dev, lead + (K,) if cfg.conf_per_frame else lead[len(lead if out_lead is None else out_lead):] + (K,))
    ins = [_dev(j3d, "j3d", dev, lead + (K, 3)), conf_p, *_param_ptrs(model, starts, global_orient, body_pose, betas, transl)]
    want_grad = False
    if world is not None:
        preserve_pose, transl_prior_target, want_grad = world
        ins += [_dev(preserve_pose, "preserve_pose", dev, (starts, _param_widths(model)[1])),
                _dev(transl_prior_target, "transl_prior_target", dev, (starts, 3))]
    out = _fit_outputs(model, lead if out_lead is None else out_lead, want_grad)
    outs = [_ptr(out[k]) for k in PARAM_KEYS + ("loss",)]
    if world is not None:
        outs.append(_ptr(out.get("grad")))
    _launch(name, dev, model.handle, prior.handle, C.byref(cfg), *head, K, _np_ptr(idx), *ins, *outs, *tail)
    return out


def fit_world(model: NativeModel, prior: NativePrior, cfg: FitConfigC, model_joint_index: Sequence[int],
              j3d: torch.Tensor, conf: Optional[torch.Tensor], global_orient: torch.Tensor, body_pose: torch.Tensor,
              betas: torch.Tensor, transl: torch.Tensor, preserve_pose: Optional[torch.Tensor] = None,
              want_grad: bool = False, transl_prior_target: Optional[torch.Tensor] = None):
    """Launch the fused fit on the current stream; returns a dict of device tensors."""
    B = j3d.shape[0]
    return _fit_call("k2b_fit_world", model, prior, cfg, (B,), _joint_index(model_joint_index, j3d.shape[1]), (B,), B,
                     j3d, conf, global_orient, body_pose, betas, transl, world=(preserve_pose, transl_prior_target, want_grad))


def fit_image(model: NativeModel, prior: NativePrior, cfg: FitConfigC, model_joint_index: Sequence[int],
              keypoints: torch.Tensor, conf: Optional[torch.Tensor], global_orient: torch.Tensor, body_pose: torch.Tensor,
              betas: torch.Tensor, transl: torch.Tensor, preserve_pose: Optional[torch.Tensor] = None,
              want_grad: bool = False, transl_prior_target: Optional[torch.Tensor] = None):
    """Independent frames of 2D keypoints (``k2b_fit_image``): ``fit_world`` under ``cfg.projection = 1`` that also takes surface
    targets (model indices >= J: extra joints, landmarks) through the projected surface kernel.  `keypoints` (B, K, 3): rows
    (u - cx, v - cy, ignored)."""
    B = keypoints.shape[0]
    return _fit_call("k2b_fit_image", model, prior, cfg, (B,), _joint_index(model_joint_index, keypoints.shape[1]), (B,), B,
                     keypoints, conf, global_orient, body_pose, betas, transl, world=(preserve_pose, transl_prior_target, want_grad))


def camera_table(cameras) -> C.Array:
    """Host table of ``CameraC`` from rows ``(rotation (3,3) or (9,), translation (3,), focal (2,))``; values are rounded to
    float32 here and checked by the entry."""
    table = (CameraC * len(cameras))()
    for slot, (rotation, translation, focal) in zip(table, cameras):
        slot.rotation[:] = np.asarray(rotation, dtype=np.float64).reshape(9).astype(np.float32).tolist()
        slot.translation[:] = np.asarray(translation, dtype=np.float64).reshape(3).astype(np.float32).tolist()
        slot.focal[:] = np.asarray(focal, dtype=np.float64).reshape(2).astype(np.float32).tolist()
    return table


def fit_multiview(model: NativeModel, prior: NativePrior, cfg: FitConfigC, cameras, model_joint_index: Sequence[int],
                  keypoints: torch.Tensor, conf: Optional[torch.Tensor], global_orient: torch.Tensor, body_pose: torch.Tensor,
                  betas: torch.Tensor, transl: torch.Tensor, preserve_pose: Optional[torch.Tensor] = None,
                  want_grad: bool = False, transl_prior_target: Optional[torch.Tensor] = None):
    """Independent frames of 2D keypoints seen by C calibrated cameras (``k2b_fit_multiview``): `cameras` a ``CameraC`` array
    (``camera_table``) or rows for one, `keypoints` (B, C, K, 3) rows (u - cx_c, v - cy_c, ignored), `conf` (C, K) or, with
    ``cfg.conf_per_frame``, (B, C, K); `transl` is the body's world translation.  One launch for all iterations."""
    table = cameras if isinstance(cameras, C.Array) else camera_table(cameras)
    if keypoints.dim() != 4:
        raise ValueError(f"keypoints must be (B, C, K, 3), got {tuple(keypoints.shape)}")
    B, V = keypoints.shape[0], keypoints.shape[1]
    if V != len(table):
        raise ValueError(f"keypoints has {V} views for {len(table)} cameras")
    return _fit_call("k2b_fit_multiview", model, prior, cfg, (B, V, table), _joint_index(model_joint_index, keypoints.shape[2]), (B, V), B,
                     keypoints, conf, global_orient, body_pose, betas, transl, world=(preserve_pose, transl_prior_target, want_grad),
                     out_lead=(B,))


def fit_world_lbfgs(model: NativeModel, prior: NativePrior, cfg: FitConfigC, model_joint_index: Sequence[int],
                    j3d: torch.Tensor, conf: Optional[torch.Tensor], global_orient: torch.Tensor, body_pose: torch.Tensor,
                    betas: torch.Tensor, transl: torch.Tensor, *, max_iter: int, lr: float,
                    preserve_pose: Optional[torch.Tensor] = None, transl_prior_target: Optional[torch.Tensor] = None,
                    want_grad: bool = False, history_size: int = 100, tolerance_grad: float = 1e-7,
                    tolerance_change: float = 1e-9):
    """The L-BFGS branch on the device (``k2b_fit_world_lbfgs``): per frame ``torch.optim.LBFGS(max_iter, lr,
    line_search_fn="strong_wolfe").step(closure)`` with this library's evaluate-only launch as the closure and the optimiser's
    state machine in a kernel of its own; only launches are queued on the current stream.  Returns the dict of ``fit_world``
    (``loss`` = the loss at the result, ``grad`` with `want_grad`)."""
    B = j3d.shape[0]
    return _fit_call("k2b_fit_world_lbfgs", model, prior, cfg, (B,), _joint_index(model_joint_index, j3d.shape[1]), (B,), B,
                     j3d, conf, global_orient, body_pose, betas, transl,
                     tail=(int(max_iter), *_lbfgs_tail(history_size, lr, tolerance_grad, tolerance_change)),
                     world=(preserve_pose, transl_prior_target, want_grad))


def fit_sequence_lbfgs(model: NativeModel, prior: NativePrior, cfg: FitConfigC, first_iters: int, followup_iters: int,
                       model_joint_index: Sequence[int], j3d: torch.Tensor, conf: Optional[torch.Tensor],
                       global_orient: torch.Tensor, body_pose: torch.Tensor, betas: torch.Tensor, transl: torch.Tensor, *, lr: float,
                       history_size: int = 100, tolerance_grad: float = 1e-7, tolerance_change: float = 1e-9):
    """ONE warm-start sequence under the L-BFGS branch (``k2b_fit_sequence_lbfgs``): ``j3d`` (T, K, 3), start (1, ...) of frame
    0; every later frame starts from its predecessor's result with ``cfg.pose_preserve_weight``; returns (T, ...) tensors."""
    T = j3d.shape[0]
    return _fit_call("k2b_fit_sequence_lbfgs", model, prior, cfg, (T,), _joint_index(model_joint_index, j3d.shape[1]), (T,), 1,
                     j3d, conf, global_orient, body_pose, betas, transl,
                     tail=(int(first_iters), int(followup_iters), *_lbfgs_tail(history_size, lr, tolerance_grad, tolerance_change)))


def fit_sequence(model: NativeModel, prior: NativePrior, cfg: FitConfigC, followup_iters: int,
                 model_joint_index: Sequence[int], j3d: torch.Tensor, conf: Optional[torch.Tensor],
                 global_orient: torch.Tensor, body_pose: torch.Tensor, betas: torch.Tensor, transl: torch.Tensor):
    """Warm-start chains in one launch (``k2b_fit_sequence``): ``j3d`` (S, T, K, 3), start parameters (S, ...) of every
    sequence's first frame; returns (S, T, ...) tensors.  ``cfg.num_iters`` iterations for frame 0, ``followup_iters``
    for the others, ``cfg.pose_preserve_weight`` on frames >= 1."""
    S, T = j3d.shape[0], j3d.shape[1]
    return _fit_call("k2b_fit_sequence", model, prior, cfg, (S, T, int(followup_iters)),
                     _joint_index(model_joint_index, j3d.shape[2]), (S, T), S, j3d, conf, global_orient, body_pose, betas, transl)


def ragged_offsets(lengths) -> np.ndarray:
    """Exclusive prefix sums of per-sequence frame counts (int32): sequence s owns packed rows offsets[s] .. + lengths[s]."""
    L = _host_i32(np.asarray(lengths).reshape(-1))
    out = np.zeros(L.shape, dtype=np.int32)
    if L.size > 1:
        out[1:] = np.cumsum(L[:-1], dtype=np.int64).astype(np.int32)
    return out


def _fit_sequences_call(name, model, prior, cfg, followup, model_joint_index, lengths, offsets, j3d, *params, tail=(), views=0):
    """Shared body of the ragged entries: host int32 lengths / offsets checked against the packed frames, then the fit call
    with (S, lengths, offsets, *`followup`) in front.  `views` > 0: the packed frames are (sum T, views, K, 3)."""
    L = _host_i32(np.asarray(lengths).reshape(-1))
    O = ragged_offsets(L) if offsets is None else _host_i32(np.asarray(offsets).reshape(-1))
    S, N = int(L.shape[0]), int(j3d.shape[0])
    idx = _joint_index(model_joint_index, int(j3d.shape[2 if views else 1]))
    if O.shape != (S,):
        raise ValueError(f"offsets has {O.shape[0]} entries for {S} sequences")
    if S and int(L.astype(np.int64).sum()) != N and (L >= 0).all():
        raise ValueError(f"lengths sum to {int(L.astype(np.int64).sum())}, j3d has {N} frames")
    return _fit_call(name, model, prior, cfg, (S, _np_ptr(L), _np_ptr(O), *followup), idx, (N, views) if views else (N,), S, j3d, *params,
                     tail=tail, out_lead=(N,) if views else None)


def fit_sequences(model: NativeModel, prior: NativePrior, cfg: FitConfigC, followup_iters: int,
                  model_joint_index: Sequence[int], lengths, j3d: torch.Tensor, conf: Optional[torch.Tensor],
                  global_orient: torch.Tensor, body_pose: torch.Tensor, betas: torch.Tensor, transl: torch.Tensor, offsets=None):
    """Warm-start chains of different lengths side by side, Adam branch (``k2b_fit_sequences``, ONE launch): ``j3d`` packed
    (sum T, K, 3), ``lengths`` (S,), start parameters (S, ...) of every sequence's first frame; returns packed (sum T, ...)
    tensors in the caller's order.  Sequence s equals ``fit_sequence`` on it alone, bit for bit."""
    return _fit_sequences_call("k2b_fit_sequences", model, prior, cfg, (int(followup_iters),), model_joint_index, lengths,
                               offsets, j3d, conf, global_orient, body_pose, betas, transl)


def fit_image_sequences(model: NativeModel, prior: NativePrior, cfg: FitConfigC, followup_iters: int, followup_freeze_betas: bool,
                        model_joint_index: Sequence[int], lengths, keypoints: torch.Tensor, conf: Optional[torch.Tensor],
                        global_orient: torch.Tensor, body_pose: torch.Tensor, betas: torch.Tensor, transl: torch.Tensor, offsets=None):
    """Warm-start chains over 2D keypoints (``k2b_fit_image_sequences``, ONE launch): ``fit_sequences`` under the projected joint
    term.  ``cfg.projection`` must be 1; ``keypoints`` packed (sum T, K, 3) rows ``(u - cx, v - cy, ignored)``; ``transl`` is the
    camera translation; with `followup_freeze_betas` the frames after a sequence's first hold its shape.  Returns the dict of
    ``fit_sequences``."""
    return _fit_sequences_call("k2b_fit_image_sequences", model, prior, cfg, (int(followup_iters), int(bool(followup_freeze_betas))),
                               model_joint_index, lengths, offsets, keypoints, conf, global_orient, body_pose, betas, transl)


def fit_multiview_sequences(model: NativeModel, prior: NativePrior, cfg: FitConfigC, followup_iters: int, followup_freeze_betas: bool,
                            cameras, model_joint_index: Sequence[int], lengths, keypoints: torch.Tensor, conf: Optional[torch.Tensor],
                            global_orient: torch.Tensor, body_pose: torch.Tensor, betas: torch.Tensor, transl: torch.Tensor, offsets=None):
    """Warm-start chains over videos of a calibrated rig (``k2b_fit_multiview_sequences``, ONE launch): ``fit_image_sequences``
    under the joint term of ``fit_multiview``.  `cameras` a ``CameraC`` array (``camera_table``) or rows for one, shared by all
    sequences and frames; ``keypoints`` packed (sum T, C, K, 3) rows ``(u - cx_c, v - cy_c, ignored)``; `conf` (C, K) or, with
    ``cfg.conf_per_frame``, (sum T, C, K); ``transl`` is the body's world translation.  Returns the dict of ``fit_sequences``."""
    table = cameras if isinstance(cameras, C.Array) else camera_table(cameras)
    if keypoints.dim() != 4:
        raise ValueError(f"keypoints must be (sum T, C, K, 3), got {tuple(keypoints.shape)}")
    V = int(keypoints.shape[1])
    if V != len(table):
        raise ValueError(f"keypoints has {V} views for {len(table)} cameras")
    return _fit_sequences_call("k2b_fit_multiview_sequences", model, prior, cfg,
                               (int(followup_iters), int(bool(followup_freeze_betas)), V, table), model_joint_index, lengths, offsets,
                               keypoints, conf, global_orient, body_pose, betas, transl, views=V)


def fit_sequences_lbfgs(model: NativeModel, prior: NativePrior, cfg: FitConfigC, first_iters: int, followup_iters: int,
                        model_joint_index: Sequence[int], lengths, j3d: torch.Tensor, conf: Optional[torch.Tensor],
                        global_orient: torch.Tensor, body_pose: torch.Tensor, betas: torch.Tensor, transl: torch.Tensor, *,
                        lr: float, history_size: int = 100, tolerance_grad: float = 1e-7, tolerance_change: float = 1e-9,
                        offsets=None):
    """The default sequence mode (L-BFGS, warm start) for S sequences of different lengths (``k2b_fit_sequences_lbfgs``, ONE
    launch; ``NotImplementedError`` where it does not apply: SMPL-H / SMPL-X, surface targets).  Arguments and result as
    ``fit_sequences``; sequence s equals ``fit_sequence_lbfgs`` on it alone, bit for bit."""
    return _fit_sequences_call(
        "k2b_fit_sequences_lbfgs", model, prior, cfg, (), model_joint_index, lengths, offsets, j3d, conf, global_orient,
        body_pose, betas, transl,
        tail=(int(first_iters), int(followup_iters), *_lbfgs_tail(history_size, lr, tolerance_grad, tolerance_change)))


def sequence_order(lengths, offsets=None) -> np.ndarray:
    """The chain-slot order of ``k2b_fit_sequences*`` (``k2b_sequence_order``, host only): the sequences with frames, longest
    first, ties in the caller's order."""
    L = _host_i32(np.asarray(lengths).reshape(-1))
    O = ragged_offsets(L) if offsets is None else _host_i32(np.asarray(offsets).reshape(-1))
    order = np.zeros(max(int(L.shape[0]), 1), dtype=np.int32)
    n = C.c_int32(0)
    _check(load_library().k2b_sequence_order(int(L.shape[0]), _np_ptr(L), _np_ptr(O), _np_ptr(order), C.byref(n)),
           "k2b_sequence_order")
    return order[: n.value].copy()


def shape_pass_lbfgs(model: NativeModel, prior: NativePrior, cfg: FitConfigC, seq_offsets: torch.Tensor,
                     model_joint_index: Sequence[int], j3d: torch.Tensor, conf: Optional[torch.Tensor], global_orient: torch.Tensor,
                     body_pose: torch.Tensor, root_targets: torch.Tensor, root_joint: int, betas: torch.Tensor, *, max_iter: int,
                     lr: float, history_size: int = 100, tolerance_grad: float = 1e-7, tolerance_change: float = 1e-9):
    """The batched shape pre-pass (``k2b_shape_pass_lbfgs``): ``seq_offsets`` device int32 (S + 1,), per-frame targets (N, K, 3),
    confidences (N, K), pose (N, 3) / (N, D), target roots (N, 3); ``betas`` (S, nb) start; returns the fitted (S, nb)."""
    dev = model.device
    N, K = int(j3d.shape[0]), int(j3d.shape[1])
    S, nb = int(betas.shape[0]), int(betas.shape[1])
    D = 3 * (model.num_joints - 1)
    idx = _joint_index(model_joint_index, K)
    if not isinstance(seq_offsets, torch.Tensor) or seq_offsets.dtype != torch.int32 or seq_offsets.device != dev \
            or tuple(seq_offsets.shape) != (S + 1,) or not seq_offsets.is_contiguous():
        raise ValueError("seq_offsets must be a contiguous int32 device tensor of S + 1 entries")
    out = _output("betas", (S, nb), dev)
    _launch("k2b_shape_pass_lbfgs", dev, model.handle, prior.handle, C.byref(cfg), S, _ptr(seq_offsets), N, K, _np_ptr(idx),
            _dev(j3d, "j3d", dev, (N, K, 3)), _dev(conf, "conf", dev, (N, K)), _dev(global_orient, "global_orient", dev, (N, 3)),
            _dev(body_pose, "body_pose", dev, (N, D)), _dev(root_targets, "root_targets", dev, (N, 3)), int(root_joint), nb,
            _dev(betas, "betas", dev, (S, nb)), _ptr(out), int(max_iter),
            *_lbfgs_tail(history_size, lr, tolerance_grad, tolerance_change))
    return out


# ---- development: the device L-BFGS state machine fed a caller's closure results (k2b_debug_lbfgs_step) ------------------------
# columns of a frame's two scalar state rows, in the order of csrc/k2b_lbfgs_plan.h's SD_* / SI_* enumerators
LBFGS_STATE_DOUBLES = ("loss", "prev_loss", "hdiag", "t", "t_prev", "f_prev", "gtd_prev", "f0", "gtd0", "dnorm", "bt0", "bt1", "bf0",
                       "bf1", "bg0", "bg1", "ro")
LBFGS_STATE_INTS = ("phase", "nold", "niter", "evals", "ls_iter", "max_ls", "ls_evals", "first", "low", "insuf", "head")


def lbfgs_debug_layout(num_frames: int, num_params: int, history: int) -> dict:
    """``k2b_debug_lbfgs_state_layout`` (host only): bytes of the optimiser's state buffer, the offsets of its integer and
    vector blocks and the row lengths of the two scalar blocks."""
    b, oi, ov, nd, ni = _i64(0), _i64(0), _i64(0), _i32(0), _i32(0)
    _check(load_library().k2b_debug_lbfgs_state_layout(int(num_frames), int(num_params), int(history), C.byref(b), C.byref(oi),
                                                       C.byref(ov), C.byref(nd), C.byref(ni)), "k2b_debug_lbfgs_state_layout")
    return {"bytes": b.value, "offset_ints": oi.value, "offset_vectors": ov.value, "doubles_per_frame": nd.value,
            "ints_per_frame": ni.value}


class LbfgsDebug:
    """B device optimisers driven one closure result at a time (``k2b_debug_lbfgs_step``): ``params`` are the four parameter
    arrays (B, 3 | D | NB | 3) holding the start; after ``step(loss, grad)`` they hold the next point to evaluate.  The history
    is cut to ``min(history_size, max_iter)`` slots as the fit entries cut it."""

    def __init__(self, global_orient, body_pose, betas, transl, *, max_iter: int, lr: float, history_size: int = 100,
                 tolerance_grad: float = 1e-7, tolerance_change: float = 1e-9, max_staged_pairs: int = -1):
        self.device = require_device(global_orient.device if isinstance(global_orient, torch.Tensor) else None)
        B = int(global_orient.shape[0])
        self.B, self.D, self.NB = B, int(body_pose.shape[1]), int(betas.shape[1])
        self.P = 3 + self.D + self.NB + 3
        self.params = (global_orient, body_pose, betas, transl)
        for t, k, w in zip(self.params, PARAM_KEYS, (3, self.D, self.NB, 3)):
            _dev(t, k, self.device, (B, w))
        self.max_iter, self.history = int(max_iter), min(int(history_size), max(int(max_iter), 1))
        self.tail = (float(lr), float(tolerance_grad), float(tolerance_change))
        self.max_staged_pairs = int(max_staged_pairs)
        self.layout = lbfgs_debug_layout(B, self.P, self.history)
        self.state = torch.zeros(max(self.layout["bytes"], 16), dtype=torch.uint8, device=self.device)     # zeroed: phase INIT

    def _call(self, params, state, loss, grad, finalize):
        _launch("k2b_debug_lbfgs_step", self.device, self.B, self.D, self.NB, *(_ptr(t) for t in params), loss, grad, self.max_iter,
                self.history, *self.tail, _ptr(state), int(state.numel()), int(finalize), self.max_staged_pairs)

    def step(self, loss: torch.Tensor, grad: torch.Tensor) -> None:
        """Consume the closure's result (B,), (B, P) at the point the parameter arrays hold."""
        self._call(self.params, self.state, _dev(loss, "loss", self.device, (self.B,)), _dev(grad, "grad", self.device, (self.B, self.P)),
                   0)

    def finalized(self):
        """The accepted point of every frame, from a finalize call on a COPY of the state and the parameters (the run is not
        disturbed): (B, P) tensor in the packed layout."""
        params, state = tuple(t.clone() for t in self.params), self.state.clone()
        self._call(params, state, None, None, 1)
        return torch.cat(params, dim=1)

    def point(self) -> torch.Tensor:
        """The parameter arrays as one (B, P) tensor in the packed layout: the next point to evaluate."""
        return torch.cat(self.params, dim=1)

    def read_state(self) -> dict:
        """The per-frame scalars as named host arrays: every name of LBFGS_STATE_INTS (int32 (B,)) and of LBFGS_STATE_DOUBLES
        (float64 (B,); ``ro``: (B, history))."""
        raw = self.state.cpu().numpy()
        L, B = self.layout, self.B
        sd = raw[: B * L["doubles_per_frame"] * 8].view(np.float64).reshape(B, L["doubles_per_frame"])
        si = raw[L["offset_ints"]: L["offset_ints"] + B * L["ints_per_frame"] * 4].view(np.int32).reshape(B, L["ints_per_frame"])
        if L["ints_per_frame"] != len(LBFGS_STATE_INTS) or L["doubles_per_frame"] != len(LBFGS_STATE_DOUBLES) - 1 + self.history:
            raise RuntimeError("libk2b.so's L-BFGS state rows differ from native.LBFGS_STATE_*")
        out = {k: si[:, i].copy() for i, k in enumerate(LBFGS_STATE_INTS)}
        out.update({k: sd[:, i].copy() for i, k in enumerate(LBFGS_STATE_DOUBLES[:-1])})
        out["ro"] = sd[:, len(LBFGS_STATE_DOUBLES) - 1:].copy()
        return out


def angular_error_deg(pred_rotvec: torch.Tensor, gt_rotvec: torch.Tensor) -> torch.Tensor:
    """Geodesic angle in degrees between pairs of axis-angle rotations, (..., 3) x (..., 3) -> (...)
    (``k2b_angular_error_deg``; launched on the current stream of the tensors' device)."""
    dev = require_device(pred_rotvec.device if isinstance(pred_rotvec, torch.Tensor) else None)
    if tuple(pred_rotvec.shape) != tuple(gt_rotvec.shape) or pred_rotvec.shape[-1] != 3:
        raise ValueError(f"expected two (...,3) tensors of equal shape, got {tuple(pred_rotvec.shape)} and {tuple(gt_rotvec.shape)}")
    n = pred_rotvec.numel() // 3
    out = _output("deg", pred_rotvec.shape[:-1], dev)
    _launch("k2b_angular_error_deg", dev, n, _dev(pred_rotvec, "pred_rotvec", dev), _dev(gt_rotvec, "gt_rotvec", dev),
            _ptr(out) if n else None)
    return out


POINT_ALIGN_MODES = {"none": 0, "translation": 1, "rigid": 2, "similarity": 3}


def point_error(pred: torch.Tensor, gt: torch.Tensor, *, weights: Optional[torch.Tensor] = None, align: str = "none",
                per_point: bool = False, transform: bool = False):
    """Weighted mean distance between two point sets per frame after an alignment, (..., N, 3) x (..., N, 3) -> (...)
    (``k2b_point_error``; launched on the current stream of the tensors' device).  ``align``: ``"none"``, ``"translation"``,
    ``"rigid"`` (Kabsch) or ``"similarity"`` (Umeyama, PA-MPJPE).  ``weights``: ``(N,)`` shared by all frames or ``(..., N)``
    per frame, non-negative.  With ``per_point`` / ``transform`` the result is a tuple ``(err, [distances (..., N)],
    [transforms (..., 13): s, R row-major, t])``."""
    dev = require_device(pred.device if isinstance(pred, torch.Tensor) else None)
    if align not in POINT_ALIGN_MODES:
        raise ValueError(f"align must be one of {sorted(POINT_ALIGN_MODES)}, got {align!r}")
    if tuple(pred.shape) != tuple(gt.shape) or pred.dim() < 2 or pred.shape[-1] != 3 or pred.shape[-2] < 1:
        raise ValueError(f"expected two (...,N,3) tensors of equal shape with N >= 1, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    lead, N = tuple(pred.shape[:-2]), int(pred.shape[-2])
    B = int(np.prod(lead, dtype=np.int64))
    per_frame = 0
    if weights is not None:
        if tuple(weights.shape) == lead + (N,) and lead:
            per_frame = 1
        elif tuple(weights.shape) != (N,):
            raise ValueError(f"weights has shape {tuple(weights.shape)}, expected {(N,)} or {lead + (N,)}")
    err = _output("err", lead, dev)
    dist = _output("per_point", lead + (N,), dev) if per_point else None
    tf = _output("transform", lead + (13,), dev) if transform else None
    _launch("k2b_point_error", dev, B, N, _dev(pred, "pred", dev), _dev(gt, "gt", dev), _dev(weights, "weights", dev), per_frame,
            POINT_ALIGN_MODES[align], _ptr(err) if B else None, _ptr(dist) if B else None, _ptr(tf) if B else None)
    extra = tuple(t for t in (dist, tf) if t is not None)
    return (err,) + extra if extra else err


def _term_call(name, model: NativeModel, idx: np.ndarray, targets, conf, conf_shape, flags, sigma, joint_loss_weight, *params,
               focal=None):
    """Shared body of the stand-alone joint-loss terms: loss (B,) and gradient (B, P) in the packed layout.  `focal`: the host
    (fx, fy) pair of the projected form, passed behind the weight."""
    dev, B, T = model.device, targets.shape[0], idx.shape[0]
    focal_np = None if focal is None else _host_f32(np.asarray(focal, dtype=np.float64).reshape(2))
    ins = [_dev(targets, "targets", dev, (B, T, 3)), _dev(conf, "conf", dev, conf_shape), *flags, float(sigma),
           float(joint_loss_weight), *(() if focal_np is None else (_np_ptr(focal_np),)), *_param_ptrs(model, B, *params)]
    loss = _output("loss", (B,), dev)
    grad = _output("grad", (B, sum(_param_widths(model))), dev)
    _launch(name, dev, model.handle, B, T, _np_ptr(idx), *ins, _ptr(loss), _ptr(grad))
    return loss, grad


def vertex_term(model: NativeModel, extra_index: Sequence[int], targets: torch.Tensor, conf: Optional[torch.Tensor],
                sigma: float, joint_loss_weight: float, global_orient: torch.Tensor, body_pose: torch.Tensor,
                betas: torch.Tensor, transl: torch.Tensor):
    """Loss (B,) and gradient (B, P) of the joint-loss term of vertex-selected joints (``k2b_vertex_term``)."""
    E = targets.shape[1]
    return _term_call("k2b_vertex_term", model, _joint_index(extra_index, E, "extra_index"), targets, conf, (E,), (),
                      sigma, joint_loss_weight, global_orient, body_pose, betas, transl)


def surface_term(model: NativeModel, model_joint_index: Sequence[int], targets: torch.Tensor, conf: Optional[torch.Tensor],
                 sigma: float, joint_loss_weight: float, global_orient: torch.Tensor, body_pose: torch.Tensor,
                 betas: torch.Tensor, transl: torch.Tensor):
    """Loss (B,) and gradient (B, P) of the joint-loss term of surface targets - extra joints and landmarks, given as model
    joint indices in [J, J+E+L) - (``k2b_surface_term``).  `conf`: (T,), (B, T) per frame, or None."""
    B, T = targets.shape[0], targets.shape[1]
    per_frame = conf is not None and conf.dim() == 2
    return _term_call("k2b_surface_term", model, _joint_index(model_joint_index, T), targets, conf,
                      (B, T) if per_frame else (T,), (1 if per_frame else 0,), sigma, joint_loss_weight,
                      global_orient, body_pose, betas, transl)


def surface_term_image(model: NativeModel, model_joint_index: Sequence[int], targets: torch.Tensor, conf: Optional[torch.Tensor],
                       sigma: float, joint_loss_weight: float, focal, global_orient: torch.Tensor, body_pose: torch.Tensor,
                       betas: torch.Tensor, transl: torch.Tensor):
    """``surface_term`` under perspective projection (``k2b_surface_term_image``): `targets` (B, T, 3) rows (u - cx, v - cy,
    ignored) in centred pixels, `sigma` in pixels, `focal` = (fx, fy)."""
    B, T = targets.shape[0], targets.shape[1]
    per_frame = conf is not None and conf.dim() == 2
    return _term_call("k2b_surface_term_image", model, _joint_index(model_joint_index, T), targets, conf,
                      (B, T) if per_frame else (T,), (1 if per_frame else 0,), sigma, joint_loss_weight,
                      global_orient, body_pose, betas, transl, focal=focal)


def adam_step(params: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, step_size: float,
              beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
    """In-place ``torch.optim.Adam`` single-tensor step ``step`` (1-based) on a flat float32 block (``k2b_adam_step``)."""
    dev = require_device(params.device)
    n = params.numel()
    for name, t in (("grad", grad), ("m", m), ("v", v)):
        if t.numel() != n:
            raise ValueError(f"{name} has {t.numel()} elements, params {n}")
    _launch("k2b_adam_step", dev, n, _dev(params, "params", dev), _dev(grad, "grad", dev), _dev(m, "m", dev), _dev(v, "v", dev),
            int(step), float(step_size), float(beta1), float(beta2), float(eps))


class NativeIkgat(_Handle):
    """Owner of a ``k2b_ikgat`` handle: the IK-GAT regressor's packed weights and graph in HBM
    (layout: ``include/k2b.h``, ``k2b_ikgat_create``)."""

    _destroy = "k2b_ikgat_destroy"

    def __init__(self, parents, weights, input_dim: int, hidden_dim: int, num_layers: int, num_heads: int, device=None):
        self.device = require_device(device)
        par = _host_i32(parents).reshape(-1)
        w = _host_f32(weights).reshape(-1)
        self.num_joints, self.input_dim = int(par.shape[0]), int(input_dim)
        self.hidden_dim, self.num_layers, self.num_heads = int(hidden_dim), int(num_layers), int(num_heads)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(load_library().k2b_ikgat_create(C.byref(self._h), self.num_joints, self.input_dim, self.hidden_dim,
                                                   self.num_layers, self.num_heads, _np_ptr(par), _np_ptr(w), int(w.size)),
                   "k2b_ikgat_create")

    def predict(self, positions: torch.Tensor, quat_in: Optional[torch.Tensor] = None, chain: bool = False) -> torch.Tensor:
        """(T, J, 3) positions [+ (T, J, 4) xyzw quaternions] -> (T, J, 4) quaternions on the device.  ``chain``: frame t > 0
        takes frame t-1's output as its input quaternions (one launch); only ``quat_in[0]`` is read, so (1, J, 4) will do."""
        dev, J = self.device, self.num_joints
        if positions.dim() != 3 or positions.shape[1:] != (J, 3):
            raise ValueError(f"positions has shape {tuple(positions.shape)}, the network expects (T, {J}, 3)")
        T = int(positions.shape[0])
        pos = _dev(positions, "positions", dev)
        q = None
        if self.input_dim == 9:
            if quat_in is None:
                raise ValueError("the pos-rot6 network needs input quaternions")
            q = _dev(quat_in, "quat_in", dev)
            if quat_in.dim() != 3 or quat_in.shape[1:] != (J, 4) or quat_in.shape[0] not in ((1, T) if chain else (T,)):
                raise ValueError(f"quat_in has shape {tuple(quat_in.shape)}, expected ({T}, {J}, 4)"
                                 + (" or (1, J, 4) in chain mode" if chain else ""))
        out = _output("quaternions", (T, J, 4), dev)
        _launch("k2b_ikgat_predict", dev, self._h, T, pos, q, 1 if chain else 0, _ptr(out))
        return out
