"""Host side of the projected joint term: the fit configuration's new fields in the header, the library and the ctypes
mirror, their defaults, the ABI version and the package's new public function.  No GPU."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _header_fields():
    text = (ROOT / "include" / "k2b.h").read_text()
    body = re.search(r"typedef struct k2b_fit_config \{(.*?)\} k2b_fit_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"\b(?:int32_t|float|double)\s+(\w+)(?:\[\d+\])?\s*;", body)


def test_the_header_appends_projection_and_focal_behind_num_betas_prior():
    fields = _header_fields()
    assert fields[-3:] == ["num_betas_prior", "projection", "focal"]


def test_the_mirror_names_the_headers_fields_in_order():
    from keypoints2body_amd import native
    assert [n for n, _ in native.FitConfigC._fields_] == _header_fields()
    by_name = dict(native.FitConfigC._fields_)
    assert by_name["projection"] is C.c_int32 and by_name["focal"] is C.c_float * 2


def test_defaults_size_and_version():
    from keypoints2body_amd import native
    lib = native.load_library()
    assert lib.k2b_fit_config_size() == C.sizeof(native.FitConfigC)
    cfg = native.FitConfigC()
    cfg.projection, cfg.focal[0], cfg.focal[1] = 7, 1.0, 2.0
    lib.k2b_fit_config_default(C.byref(cfg))
    assert cfg.projection == 0 and tuple(cfg.focal) == (0.0, 0.0)
    assert lib.k2b_version() >> 16 == 1 and (lib.k2b_version() & 0xffff) >= 7      # the minor version grew with the fields


def test_the_package_exports_the_image_space_entry():
    import keypoints2body_amd as pkg
    from keypoints2body_amd.api.image import optimize_params_frame_2d
    from keypoints2body_amd.core.fitters.common import FitterBase
    from keypoints2body_amd.core.fitters.image_space import ImageSpaceFitter
    assert pkg.optimize_params_frame_2d is optimize_params_frame_2d and "optimize_params_frame_2d" in pkg.__all__
    assert issubclass(ImageSpaceFitter, FitterBase)
    params = inspect.signature(optimize_params_frame_2d).parameters
    for name in ("keypoints2d", "focal", "principal_point", "conf", "body_model", "model", "config", "init_params", "joint_layout"):
        assert name in params, name
    assert all(params[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("focal", "principal_point"))


def test_joints2d_stays_refused_on_the_existing_entries():
    from keypoints2body_amd.api import common
    from keypoints2body_amd.core.config import FrameOptimizeConfig
    with pytest.raises(NotImplementedError, match="joints2d"):
        common.check_request(FrameOptimizeConfig(input_type="joints2d"), "smpl")
