"""ctypes wrapper of the reference's own kernels built for the CPU (oracle/ref/).

TEST INFRASTRUCTURE ONLY.  The libraries under oracle/_ref/ are compiled from the
reference's kernel text by oracle/ref/build_ref.py; they are never committed.
tests/test_reference_text.py holds oracle/vr_oracle.c to them word for word,
tests/test_gpu_reference.py the HIP library.
"""
from __future__ import annotations

import ctypes
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (50, 50, 10)  # the reference's hard-coded volume (K:90, K:727-729)
NVOX = 50 * 50 * 10
_libs = {}


def _recipe():
    spec = importlib.util.spec_from_file_location(
        "vr_build_ref", os.path.join(_HERE, "ref", "build_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


recipe = _recipe()


def have_reference_dir() -> bool:
    return recipe.reference_present()


def available(name: str = "b32") -> bool:
    return os.path.exists(recipe.lib_path(name))


class Ref:
    """One built variant: 'b32', 'b8' (canonical, -ffp-contract=off), 'b32_fma'
    (contracted) or 'b32_exit_canary' (wrong on purpose).  The library keeps one
    bound volume at a time, like the reference's file-scope textures."""

    def __init__(self, name: str):
        L = ctypes.CDLL(recipe.lib_path(name))
        fp = ctypes.POINTER(ctypes.c_float)
        L.ref_nbins.restype = ctypes.c_int
        L.ref_set_weight_trunc.argtypes = [ctypes.c_int]
        L.ref_init.argtypes = [fp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                               ctypes.c_void_p, ctypes.c_int]
        L.ref_basic_data_processing.argtypes = [fp, fp]
        L.ref_bind_flex.argtypes = [fp, ctypes.c_int]
        L.ref_set_inv_view.argtypes = [fp]
        L.ref_render.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint] + \
            [ctypes.c_float] * 4 + [ctypes.c_int] * 4
        for f in (L.ref_set_weight_trunc, L.ref_init, L.ref_basic_data_processing,
                  L.ref_bind_flex, L.ref_set_inv_view, L.ref_render):
            f.restype = None
        self.L = L
        self.name = name
        self.nbins = int(L.ref_nbins())

    def init(self, hist, codec=None):
        """initCuda: hist float32 (10, 50, 50, nbins) or (25000, nbins); codec
        (codebook int32 (..., 4), templates (T, nbins), errors (..., slots, 2)) or None"""
        hist = np.ascontiguousarray(hist, dtype=np.float32).reshape(NVOX, self.nbins)
        if codec is None:
            self.L.ref_init(_fp(hist), None, None, 0, None, 0)
            return
        cb = np.ascontiguousarray(codec[0], dtype=np.int32).reshape(NVOX, 4)
        tp = np.ascontiguousarray(codec[1], dtype=np.float32)
        er = np.ascontiguousarray(codec[2], dtype=np.float32)
        assert tp.shape[1] == self.nbins
        slots = er.shape[-2]
        er = er.reshape(NVOX, slots, 2)
        self.L.ref_init(_fp(hist), cb.ctypes.data, tp.ctypes.data, tp.shape[0],
                        er.ctypes.data, slots)

    def basic_data_processing(self):
        """basicDataProcessing: (originalHistogramData, fractalHistogramData), each
        float32 (25000, 4) = (mean, variance, entropy, unused)"""
        o = np.zeros((NVOX, 4), np.float32)
        f = np.zeros((NVOX, 4), np.float32)
        self.L.ref_basic_data_processing(_fp(o), _fp(f))
        return o, f

    def bind_flex(self, blocks):
        blocks = np.ascontiguousarray(blocks, dtype=np.float32)
        self.L.ref_bind_flex(_fp(blocks), blocks.shape[0])

    def set_weight_trunc(self, on: bool):
        """canary only: texture filter weights truncated instead of rounded"""
        self.L.ref_set_weight_trunc(int(bool(on)))

    def render(self, params, prefill=0, volume_size=None, want_float=False):
        """render_kernel with an oracle RenderParams: RGBA8 uint32 (H, W), prefilled
        (a miss writes nothing).  want_float: also the saturated float RGBA that
        rgbaFloatToInt packed, float32 (H, W, 4), NaN where the ray missed; the
        reference computes it and never stores it, the shim's __saturatef keeps it."""
        W, H = params.width, params.height
        m = np.array(list(params.inv_view), np.float32)
        self.L.ref_set_inv_view(_fp(m))
        out = np.full((H, W), prefill, np.uint32)
        out_f = np.full((H, W, 4), np.nan, np.float32) if want_float else None
        vs = volume_size or tuple(params.m7_dims)
        self.L.ref_render(out.ctypes.data, None if out_f is None else out_f.ctypes.data, W, H,
                          params.density, params.brightness, params.transfer_offset,
                          params.transfer_scale, params.query_method,
                          int(vs[0]), int(vs[1]), int(vs[2]))
        return (out, out_f) if want_float else out


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def load(name: str = "b32") -> Ref:
    if name not in _libs:
        _libs[name] = Ref(name)
    return _libs[name]
