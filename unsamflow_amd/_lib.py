"""ctypes binding of libunsamflow_hip.so (C ABI: include/unsamflow_hip.h).

The library is the only compute path of this package: there is no CPU or
PyTorch fallback. If the library is missing or cannot be loaded, every op
raises ``RuntimeError`` (the product path fails loudly).

torch must be imported first so the library binds to the HIP runtime torch
already loaded (same SONAME ``libamdhip64.so.7``).
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path

import torch  # noqa: F401  (load torch's HIP runtime before the plugin)

_LIB_PATH = Path(os.environ.get("USF_LIB", Path(__file__).resolve().parent / "lib" / "libunsamflow_hip.so"))
ABI_VERSION = 8
PAD_ZEROS = 0
PAD_BORDER = 1

# exported symbols and their signatures; tests check the library exports all of them
_c_float_p = ctypes.c_void_p
_SIGNATURES = {
    "usf_abi_version": ([], ctypes.c_int),
    "usf_last_error_string": ([], ctypes.c_char_p),
    "usf_build_id": ([], ctypes.c_char_p),
    "usf_corr_fwd_f32": (
        [_c_float_p, _c_float_p, _c_float_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_corr_bwd_f32": (
        [_c_float_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_corr_fwd_ex_f32": (
        [_c_float_p] * 3 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, _c_float_p,
                             ctypes.c_longlong]
        + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_corr_act_mask_words": ([ctypes.c_int] * 4, ctypes.c_longlong),
    "usf_corr_fwd_workspace": ([ctypes.c_int] * 5, ctypes.c_longlong),
    "usf_corr_bwd_ex_scratch": ([ctypes.c_int] * 5, ctypes.c_longlong),
    "usf_corr_bwd_ex_f32": (
        [_c_float_p] * 3 + [ctypes.c_longlong, _c_float_p, ctypes.c_void_p, ctypes.c_float] + [_c_float_p] * 3
        + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_warp_fwd_f32": (
        [_c_float_p, _c_float_p, ctypes.c_longlong, _c_float_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_warp_fwd_up_f32": ([_c_float_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p], ctypes.c_int),
    "usf_flow_upsample_bwd_sum_f32": ([_c_float_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p], ctypes.c_int),
    "usf_warp_bwd_f32": (
        [_c_float_p, _c_float_p, ctypes.c_longlong, _c_float_p, _c_float_p, _c_float_p]
        + [ctypes.c_int] * 5
        + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_warp_bwd_ex_f32": (
        [_c_float_p, _c_float_p, ctypes.c_longlong, _c_float_p, _c_float_p, _c_float_p, ctypes.c_void_p,
         ctypes.c_longlong] + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_warp_bwd_workspace": ([ctypes.c_int] * 3, ctypes.c_longlong),
    "usf_warp_bwd_persist_f32": (
        [_c_float_p, _c_float_p, ctypes.c_longlong, _c_float_p, _c_float_p, _c_float_p, ctypes.c_void_p,
         ctypes.c_longlong] + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_warp_bwd_persist_workspace": ([ctypes.c_int] * 4, ctypes.c_longlong),
    "usf_occ_backward_persist_f32": (
        [_c_float_p, ctypes.c_longlong, _c_float_p, _c_float_p, ctypes.c_longlong] + [ctypes.c_int] * 3
        + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_occ_vis_pair_persist_f32": (
        [_c_float_p, ctypes.c_longlong, _c_float_p, _c_float_p, ctypes.c_longlong] + [ctypes.c_int] * 3
        + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_splat_map_f32": (
        [_c_float_p, ctypes.c_longlong, _c_float_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_occ_backward_f32": (
        [_c_float_p, ctypes.c_longlong, _c_float_p] + [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_occ_bidirection_f32": (
        [_c_float_p, ctypes.c_longlong, _c_float_p, ctypes.c_longlong, _c_float_p] + [ctypes.c_int] * 3
        + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_photo_loss_partials": ([ctypes.c_int] * 3, ctypes.c_int),
    "usf_photo_loss_fwd_f32": (
        [_c_float_p] * 4 + [ctypes.c_longlong, _c_float_p, _c_float_p, _c_float_p] + [ctypes.c_int] * 5
        + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_photo_loss_pair_fwd_f32": (
        [_c_float_p] * 5 + [ctypes.c_longlong, _c_float_p, _c_float_p, _c_float_p] + [ctypes.c_int] * 5
        + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_photo_loss_pyramid_partials": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int],
                                        ctypes.c_longlong),
    "usf_photo_loss_pyramid_fwd_f32": (
        [ctypes.c_int] + [ctypes.c_void_p] * 8 + [_c_float_p, ctypes.c_longlong, _c_float_p, ctypes.c_void_p]
        + [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_photo_loss_pyramid_bwd_f32": (
        [ctypes.c_int, ctypes.c_void_p, _c_float_p, _c_float_p] + [ctypes.c_void_p] * 3 + [ctypes.c_int,
                                                                                            ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_photo_loss_bwd_f32": (
        [_c_float_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_flow_upsample_f32": ([_c_float_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p], ctypes.c_int),
    "usf_flow_upsample_bwd_f32": ([_c_float_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p], ctypes.c_int),
    "usf_convex_upsample_f32": (
        [_c_float_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_convex_upsample_bwd_scratch": ([ctypes.c_int] * 3, ctypes.c_longlong),
    "usf_convex_upsample_bwd_f32": (
        [_c_float_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_convex_upsample_pyramid_f32": (
        [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_convex_upsample_pyramid_bwd_scratch": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int],
                                                ctypes.c_longlong),
    "usf_convex_upsample_pyramid_bwd_f32": (
        [ctypes.c_int] + [ctypes.c_void_p] * 5 + [_c_float_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_area_pyramid_f32": ([_c_float_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p], ctypes.c_int),
    "usf_set_variant": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "usf_device_errors": ([ctypes.c_void_p, ctypes.c_int], ctypes.c_int),
    "usf_stream_copy_f32": ([_c_float_p, _c_float_p, ctypes.c_longlong, ctypes.c_void_p], ctypes.c_int),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# the census entries (include/unsamflow_hip_census.h): the same library, their
# own header and version, so USF_ABI_VERSION and the table above stay as they are
CENSUS_API_VERSION = 1
CENSUS_SYMBOLS = {
    "usf_census_api_version": ([], ctypes.c_int),
    "usf_census_loss_partials": ([ctypes.c_int] * 3, ctypes.c_int),
    "usf_census_loss_fwd_f32": (
        [_c_float_p] * 4 + [ctypes.c_longlong, _c_float_p, _c_float_p, _c_float_p] + [ctypes.c_int] * 5
        + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_census_loss_pair_fwd_f32": (
        [_c_float_p] * 5 + [ctypes.c_longlong, _c_float_p, _c_float_p, _c_float_p] + [ctypes.c_int] * 5
        + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_census_loss_bwd_f32": ([_c_float_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p], ctypes.c_int),
    "usf_census_loss_pyramid_partials": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int],
                                         ctypes.c_longlong),
    "usf_census_loss_pyramid_fwd_f32": (
        [ctypes.c_int] + [ctypes.c_void_p] * 8 + [_c_float_p, ctypes.c_longlong, _c_float_p, ctypes.c_void_p]
        + [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_census_loss_pyramid_bwd_f32": (
        [ctypes.c_int, ctypes.c_void_p, _c_float_p, _c_float_p] + [ctypes.c_void_p] * 3 + [ctypes.c_int,
                                                                                            ctypes.c_void_p],
        ctypes.c_int,
    ),
}

# the stage-1 augmentation entries (include/unsamflow_hip_ar.h), versioned the same way
AR_API_VERSION = 1
_ar_strided = [_c_float_p] + [ctypes.c_longlong] * 3 + [_c_float_p] + [ctypes.c_longlong] * 2
AR_SYMBOLS = {
    "usf_ar_api_version": ([], ctypes.c_int),
    "usf_ar_transform_f32": (
        [_c_float_p] * 3 + [ctypes.c_longlong] + [_c_float_p] * 8 + [ctypes.c_int] * 3 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_ar_loss_partials": ([ctypes.c_int] * 3, ctypes.c_int),
    "usf_ar_loss_fwd_f32": (
        [_c_float_p] + _ar_strided + [_c_float_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_ar_loss_bwd_f32": (
        [_c_float_p] + _ar_strided + [_c_float_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
}

# the mask-feature branch's per-segment max pool and spread
# (include/unsamflow_hip_segpool.h), versioned the same way
SEGPOOL_API_VERSION = 1
SEGPOOL_MAX_K = 1024
DEVERR_SEGPOOL_BAD_ID = 4
SEGPOOL_SYMBOLS = {
    "usf_segpool_api_version": ([], ctypes.c_int),
    "usf_segpool_state_words": ([ctypes.c_int] * 3, ctypes.c_longlong),
    "usf_segpool_fwd_f32": (
        [_c_float_p] * 3 + [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_segpool_bwd_f32": (
        [_c_float_p] * 2 + [ctypes.c_void_p] + [_c_float_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
}

# the homography smoothness loss (include/unsamflow_hip_hg.h), versioned the same way
HG_API_VERSION = 1
HG_MAX_K = 1024
HG_SLOTS = 6
HG_RECORD_WORDS = 16
HG_DEFAULT_HYP = 256
HG_STATUS = ("accepted", "too few reliable", "low reliable share", "low inlier share", "degenerate", "empty slot")
DEVERR_HG_BAD_ID = 8
_hg_flow = [_c_float_p, ctypes.c_longlong, _c_float_p]
HG_SYMBOLS = {
    "usf_hg_api_version": ([], ctypes.c_int),
    "usf_hg_workspace_bytes": ([ctypes.c_int] * 5, ctypes.c_longlong),
    "usf_hg_fit_f32": (
        _hg_flow + [_c_float_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_int] * 3 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_hg_loss_partials": ([ctypes.c_int] * 3, ctypes.c_int),
    "usf_hg_loss_fwd_f32": (
        _hg_flow + [ctypes.c_void_p, ctypes.c_void_p, _c_float_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_hg_loss_bwd_f32": (
        _hg_flow + [ctypes.c_void_p, _c_float_p, _c_float_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
}

# the conv epilogues (include/unsamflow_hip_convepi.h), versioned the same way
CONVEPI_API_VERSION = 1
CONVEPI_TILE_SLOTS = 1024
CONVEPI_CHAIN = 64
CONVEPI_TARGET_WGS = 16384
CONVEPI_SYMBOLS = {
    "usf_convepi_api_version": ([], ctypes.c_int),
    "usf_convepi_fwd_f32": ([_c_float_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_void_p], ctypes.c_int),
    "usf_convepi_bwd_workspace": ([ctypes.c_int] * 4, ctypes.c_longlong),
    "usf_convepi_bwd_f32": (
        [_c_float_p, ctypes.c_longlong] + [_c_float_p] * 4 + [ctypes.c_longlong] + [ctypes.c_int] * 4
        + [ctypes.c_float, ctypes.c_void_p],
        ctypes.c_int,
    ),
}

# the key-object augmentation (include/unsamflow_hip_fakeobj.h), versioned the same way
FAKEOBJ_API_VERSION = 1
FAKEOBJ_MAX_K = 8
DEVERR_FAKEOBJ_BAD_SLOT = 16
FAKEOBJ_SYMBOLS = {
    "usf_fakeobj_api_version": ([], ctypes.c_int),
    "usf_fakeobj_paste_crop_f32": (
        [_c_float_p] * 3 + [ctypes.c_longlong] + [_c_float_p] * 4 + [ctypes.c_void_p] + [_c_float_p] * 4
        + [ctypes.c_int] * 9 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_fakeobj_push_partials": ([ctypes.c_int] * 3, ctypes.c_int),
    "usf_fakeobj_push_f32": (
        [_c_float_p] * 3 + [ctypes.c_longlong, ctypes.c_void_p] + [_c_float_p] * 4 + [ctypes.c_int] * 4
        + [ctypes.c_void_p],
        ctypes.c_int,
    ),
}

# validation on the device (include/unsamflow_hip_eval.h), versioned the same way
EVAL_API_VERSION = 1
EVAL_NACC = 12
EVAL_NMETRIC = 7
DEVERR_EVAL_BAD_SIZE = 32
EVAL_SYMBOLS = {
    "usf_eval_api_version": ([], ctypes.c_int),
    "usf_flow_resize_f32": (
        [_c_float_p, ctypes.c_longlong, ctypes.c_void_p, _c_float_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
    "usf_flow_eval_partials": ([ctypes.c_int] * 3, ctypes.c_int),
    "usf_flow_eval_f32": (
        [_c_float_p, ctypes.c_longlong, _c_float_p, ctypes.c_int, _c_float_p, ctypes.c_void_p] + [_c_float_p] * 3
        + [ctypes.c_int] * 5 + [ctypes.c_void_p],
        ctypes.c_int,
    ),
}

_lock = threading.Lock()
_lib = None
_load_error: str | None = None


def library_path() -> Path:
    return _LIB_PATH


def load() -> ctypes.CDLL:
    """Load (once) and return the plugin library; raise RuntimeError if absent."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not _LIB_PATH.exists():
            _load_error = (
                f"libunsamflow_hip.so not found at {_LIB_PATH}; build it with "
                "`python -m unsamflow_amd.build` (hipcc, gfx950)"
            )
            raise RuntimeError(_load_error)
        lib = ctypes.CDLL(str(_LIB_PATH), mode=ctypes.RTLD_LOCAL)
        for name, (argtypes, restype) in {**_SIGNATURES, **CENSUS_SYMBOLS, **AR_SYMBOLS, **SEGPOOL_SYMBOLS,
                                          **HG_SYMBOLS, **CONVEPI_SYMBOLS, **FAKEOBJ_SYMBOLS,
                                          **EVAL_SYMBOLS}.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        v = lib.usf_abi_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"libunsamflow_hip.so ABI version {v} != expected {ABI_VERSION}")
        v = lib.usf_census_api_version()
        if v != CENSUS_API_VERSION:
            raise RuntimeError(f"libunsamflow_hip.so census API version {v} != expected {CENSUS_API_VERSION}")
        v = lib.usf_ar_api_version()
        if v != AR_API_VERSION:
            raise RuntimeError(f"libunsamflow_hip.so AR API version {v} != expected {AR_API_VERSION}")
        v = lib.usf_segpool_api_version()
        if v != SEGPOOL_API_VERSION:
            raise RuntimeError(f"libunsamflow_hip.so segpool API version {v} != expected {SEGPOOL_API_VERSION}")
        v = lib.usf_hg_api_version()
        if v != HG_API_VERSION:
            raise RuntimeError(f"libunsamflow_hip.so hg API version {v} != expected {HG_API_VERSION}")
        v = lib.usf_convepi_api_version()
        if v != CONVEPI_API_VERSION:
            raise RuntimeError(f"libunsamflow_hip.so convepi API version {v} != expected {CONVEPI_API_VERSION}")
        v = lib.usf_fakeobj_api_version()
        if v != FAKEOBJ_API_VERSION:
            raise RuntimeError(f"libunsamflow_hip.so fake-object API version {v} != expected {FAKEOBJ_API_VERSION}")
        v = lib.usf_eval_api_version()
        if v != EVAL_API_VERSION:
            raise RuntimeError(f"libunsamflow_hip.so evaluation API version {v} != expected {EVAL_API_VERSION}")
        _lib = lib
        return lib


def build_id() -> str:
    """The loaded library's build id (usf_build_id; unsamflow_amd.build.build_id)."""
    return load().usf_build_id().decode()


def is_available() -> bool:
    try:
        load()
        return True
    except (RuntimeError, OSError):
        return False


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().usf_last_error_string()
        msg = msg.decode() if msg else ""
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


def stream_handle(device: torch.device) -> int:
    """hipStream_t of torch's current stream on ``device``."""
    return torch.cuda.current_stream(device).cuda_stream
