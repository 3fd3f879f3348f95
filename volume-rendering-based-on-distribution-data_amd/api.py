"""Python mirror of the reference's host/launch API (volumeRender.cpp:156-170).

The functions keep the reference's names, argument order and meaning and call
straight into libvr.so.  Device buffers are passed as torch CUDA tensors or as
raw device addresses (int).  Where the reference's checkCudaErrors /
getLastCudaError would have printed and exited (C:201-216, 1070), these
functions raise VRError.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import VR_ERR_ARG, Dim3, Extent, RenderDesc, VRError, check, check_last

PAD = 0xFFFFFFFF


def _ptr(buf) -> int:
    if buf is None:
        return 0
    if isinstance(buf, int):
        return buf
    if hasattr(buf, "data_ptr"):
        if not buf.is_cuda:
            raise ValueError("device buffer expected (a CUDA/HIP tensor)")
        if not buf.is_contiguous():
            raise ValueError("device buffer must be contiguous")
        return int(buf.data_ptr())
    raise TypeError(f"cannot take a device pointer of {type(buf)!r}")


def _extent(e) -> Extent:
    if isinstance(e, Extent):
        return e
    w, h, d = (int(v) for v in e)
    return Extent(w, h, d)


def _dim3(d) -> Dim3:
    if isinstance(d, Dim3):
        return d
    d = tuple(int(v) for v in d) + (1, 1, 1)
    return Dim3(d[0], d[1], d[2])


# ---------------------------------------------------------------- reference API

def render_kernel(gridSize, blockSize, d_output, imageW: int, imageH: int, density: float,
                  brightness: float, transferOffset: float, transferScale: float,
                  queryMethod: int, volumeSize) -> None:
    """render_kernel, K:2387-2401 (asynchronous; raises on a recorded error)."""
    _lib.load().render_kernel(_dim3(gridSize), _dim3(blockSize), _ptr(d_output), int(imageW),
                              int(imageH), float(density), float(brightness),
                              float(transferOffset), float(transferScale), int(queryMethod),
                              _extent(volumeSize))
    check_last()


def copyInvViewMatrix(invViewMatrix, sizeofMatrix: int = 48) -> None:
    """copyInvViewMatrix, K:2403-2406."""
    m = np.ascontiguousarray(np.asarray(invViewMatrix, dtype=np.float32).reshape(-1))
    if m.nbytes < sizeofMatrix:
        raise ValueError("matrix smaller than sizeofMatrix")
    _lib.load().copyInvViewMatrix(m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                  int(sizeofMatrix))
    check_last()


def initCuda(h_histogram, volumeSize, histogramSize, h_codebook=None, codebookSize=None,
             h_templates=None, templatesSize=None, h_errorsbook=None, errorsbookSize=None,
             *flexible_arrays) -> None:
    """initCuda, K:1893-2358.  h_histogram: host fp32 array of B-bin records in
    AoS order (record = x + X*(y + Y*z)).  h_codebook (int32 [..., 4]),
    h_templates (fp32 [T, B]) and h_errorsbook (fp32 [..., slots, 2]) make the
    codec volume of methods 4/5/6 resident (sizes as the reference passes them:
    codebookSize = volumeSize, templatesSize = (B, T, 1), errorsbookSize =
    (slots, rows, layers)).  flexible_arrays: the nine span-table arrays of
    arguments 10-18 (codebookSpanLow, codebookSpanHigh, flexibleCodebook,
    flexibleErrorsbook, simpleLow, simpleHigh, simpleCount, simpleHistogram,
    flexibleTemplates) at the reference's fixed sizes (vr_init_flex)."""
    h = np.ascontiguousarray(np.asarray(h_histogram, dtype=np.float32))
    L = _lib.load()
    z = Extent(0, 0, 0)
    keep = []

    def arr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a, dtype=dt))
        keep.append(a)
        return a.ctypes.data

    L.initCuda(h.ctypes.data, _extent(volumeSize), _extent(histogramSize),
               arr(h_codebook, np.int32), _extent(codebookSize) if codebookSize else z,
               arr(h_templates, np.float32), _extent(templatesSize) if templatesSize else z,
               arr(h_errorsbook, np.float32), _extent(errorsbookSize) if errorsbookSize else z,
               *_flex_initcuda_args(flexible_arrays, arr))
    check_last()


def _flex_initcuda_args(flexible_arrays, arr):
    if not flexible_arrays:
        return [None] * 9
    if len(flexible_arrays) != 9:
        raise ValueError("initCuda takes all nine flexible-block arrays or none")
    types = [np.int32] * 3 + [np.float32] + [np.int32] * 3 + [np.float32] * 2
    return [arr(a, t) for a, t in zip(flexible_arrays, types)]


def init_flex(tables: dict) -> None:
    """Make flexible-block span tables resident (methods 8/9/0; vr_init_flex).
    tables: dim, nbins, fractal_low/high/code int32 (n, 4), fractal_err float32
    (n, nbins, 2), simple_low/high int32 (m, 4), simple_count int32 (m,),
    simple_hist float32 (m, nbins, 2), templates float32 (T, nbins)."""
    keep = {}
    for k, dt in (("fractal_low", np.int32), ("fractal_high", np.int32),
                  ("fractal_code", np.int32), ("fractal_err", np.float32),
                  ("simple_low", np.int32), ("simple_high", np.int32),
                  ("simple_count", np.int32), ("simple_hist", np.float32),
                  ("templates", np.float32)):
        keep[k] = np.ascontiguousarray(tables[k], dtype=dt)
    t = _lib.FlexTables()
    t.dim, t.nbins = int(tables["dim"]), int(tables["nbins"])
    t.n_fractal, t.n_simple = keep["fractal_low"].shape[0], keep["simple_low"].shape[0]
    t.ntemplates = keep["templates"].shape[0]
    t.fractal_low, t.fractal_high = keep["fractal_low"].ctypes.data, keep["fractal_high"].ctypes.data
    t.fractal_code, t.fractal_errors = keep["fractal_code"].ctypes.data, keep["fractal_err"].ctypes.data
    t.simple_low, t.simple_high = keep["simple_low"].ctypes.data, keep["simple_high"].ctypes.data
    t.simple_count, t.simple_hist = keep["simple_count"].ctypes.data, keep["simple_hist"].ctypes.data
    t.templates = keep["templates"].ctypes.data
    check(_lib.load().vr_init_flex(ctypes.byref(t)))


def load_flex_files(span_list, fractal, simple_counts, simple_bin_ids, simple_bin_freqs,
                    templates, dim: int = 64, nbins: int = 64) -> None:
    """The reference's flexible-block files (spanList.bin, codebook0.bin, nzbCounts0.bin,
    nzbBinIds0.bin, nzbFreqs0.bin, domainList.bin; C:79-84) -> resident span tables."""
    args = [str(a).encode() for a in (span_list, fractal, simple_counts, simple_bin_ids,
                                      simple_bin_freqs, templates)]
    check(_lib.load().vr_load_flex_files(*args, int(dim), int(nbins)))


def parse_flex_files(span_list, fractal, simple_counts, simple_bin_ids, simple_bin_freqs,
                     templates, dim: int = 64, nbins: int = 64) -> dict:
    """Parse the flexible-block files on the host into the table dict init_flex takes."""
    L = _lib.load()
    sp = str(span_list).encode()
    n = L.vr_parse_span_list(sp, 0, None, None)
    if n < 0:
        raise VRError(VR_ERR_ARG, f"span list: {n}")
    sl, sh = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
    L.vr_parse_span_list(sp, n, sl.ctypes.data, sh.ctypes.data)
    fp = str(fractal).encode()
    nf = L.vr_parse_fractal_histogram(fp, sl.ctypes.data, sh.ctypes.data, n, nbins, 0,
                                      None, None, None, None)
    if nf < 0:
        raise VRError(VR_ERR_ARG, f"fractal spans: {nf}")
    t = {"dim": dim, "nbins": nbins,
         "fractal_low": np.zeros((nf, 4), np.int32), "fractal_high": np.zeros((nf, 4), np.int32),
         "fractal_code": np.zeros((nf, 4), np.int32),
         "fractal_err": np.zeros((nf, nbins, 2), np.float32)}
    L.vr_parse_fractal_histogram(fp, sl.ctypes.data, sh.ctypes.data, n, nbins, nf,
                                 t["fractal_low"].ctypes.data, t["fractal_high"].ctypes.data,
                                 t["fractal_code"].ctypes.data, t["fractal_err"].ctypes.data)
    paths = [str(p).encode() for p in (simple_counts, simple_bin_ids, simple_bin_freqs)]
    ns = L.vr_parse_simple_histogram(*paths, nbins, 0, None, None, None, None)
    if ns < 0:
        raise VRError(VR_ERR_ARG, f"simple spans: {ns}")
    t.update({"simple_low": np.zeros((ns, 4), np.int32), "simple_high": np.zeros((ns, 4), np.int32),
              "simple_count": np.zeros(ns, np.int32),
              "simple_hist": np.zeros((ns, nbins, 2), np.float32)})
    L.vr_parse_simple_histogram(*paths, nbins, ns, t["simple_low"].ctypes.data,
                                t["simple_high"].ctypes.data, t["simple_count"].ctypes.data,
                                t["simple_hist"].ctypes.data)
    tp = str(templates).encode()
    nt = L.vr_parse_templates(tp, nbins, 0, None)
    if nt <= 0:
        raise VRError(VR_ERR_ARG, f"flexible templates: {nt}")
    t["templates"] = np.zeros((nt, nbins), np.float32)
    L.vr_parse_templates(tp, nbins, nt, t["templates"].ctypes.data)
    return t


def flex_process(block: int) -> int:
    """dataProcessing with `block`-voxel blocks (vr_flex_process); returns blocks per axis."""
    return int(check(_lib.load().vr_flex_process(int(block))))


def flex_info():
    """(blocks per axis, bins, device pointer of the float4 block statistics)"""
    n, nb, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_void_p()
    check(_lib.load().vr_flex_info(ctypes.byref(n), ctypes.byref(nb), ctypes.byref(p)))
    return n.value, nb.value, p.value


def init_codec(codebook, templates, errors) -> None:
    """Make a fractal/template codec volume resident (methods 4/5/6).
    codebook int32 (nz, ny, nx, 4) = (template id, shift, flip, NE); templates fp32
    (T, B); errors fp32 (nz, ny, nx, slots, 2) = (bin id, value).  Host numpy arrays
    or CUDA tensors (copied)."""
    L = _lib.load()
    if hasattr(codebook, "data_ptr") and getattr(codebook, "is_cuda", False):
        nz, ny, nx, _ = codebook.shape
        check(L.vr_init_codec(_ptr(codebook), _extent((nx, ny, nz)), _ptr(templates),
                              int(templates.shape[0]), _ptr(errors), int(errors.shape[-2]),
                              int(templates.shape[1]), 1))
        return
    cb = np.ascontiguousarray(codebook, dtype=np.int32)
    tp = np.ascontiguousarray(templates, dtype=np.float32)
    er = np.ascontiguousarray(errors, dtype=np.float32)
    nz, ny, nx, _ = cb.shape
    check(L.vr_init_codec(cb.ctypes.data, _extent((nx, ny, nz)), tp.ctypes.data, tp.shape[0],
                          er.ctypes.data, er.shape[-2], tp.shape[1], 0))


def freeCudaBuffers() -> None:
    """freeCudaBuffers, K:2360-2385."""
    _lib.load().freeCudaBuffers()
    check_last()


def setTextureFilterMode(bLinearFilter: bool) -> None:
    """setTextureFilterMode, K:1889-1891 (no effect on methods 1/2/3/7)."""
    _lib.load().setTextureFilterMode(bool(bLinearFilter))


def basicDataProcessing() -> None:
    """basicDataProcessing, K:1798-1887: bakes the per-voxel statistics of the resident
    raw / codec volumes (originalQueryTex / fractalQueryTex, K:722-871) into float
    planes; methods 1-7 then read the planes (bit-identical to the per-step decode)."""
    _lib.load().basicDataProcessing()
    check_last()


def bake_stats() -> None:
    """vr_bake_stats: basicDataProcessing with a status (raises VRError)."""
    check(_lib.load().vr_bake_stats())


def release_stats() -> None:
    """Drop the baked planes: methods 1-7 decode the records per step again."""
    check(_lib.load().vr_release_stats())


def stats_info():
    """((d_raw, raw_plane_floats), (d_codec, codec_plane_floats)); pointer None = not baked"""
    a, c = ctypes.c_void_p(), ctypes.c_void_p()
    na, nc = ctypes.c_uint64(), ctypes.c_uint64()
    check(_lib.load().vr_stats_info(ctypes.byref(a), ctypes.byref(na), ctypes.byref(c),
                                    ctypes.byref(nc)))
    return (a.value, na.value), (c.value, nc.value)


def set_layout_budget(nbytes=None) -> None:
    """Cap the HBM the library spends on layout copies (micro-brick and
    axis-rows copies of the records, baked-plane copies; include/vr.h): None =
    the default budget, 0 = never make one."""
    check(_lib.load().vr_set_layout_budget(0xFFFFFFFFFFFFFFFF if nbytes is None else int(nbytes)))


def layout_info() -> dict:
    """Layout copies: bytes resident, copies made since load, and the time (ms)
    and size of the last one made -- the extra cost of the first frame of a view
    that needs a copy."""
    b, n = ctypes.c_uint64(), ctypes.c_int()
    ms, lb = ctypes.c_float(), ctypes.c_uint64()
    check(_lib.load().vr_layout_info(ctypes.byref(b), ctypes.byref(n), ctypes.byref(ms),
                                     ctypes.byref(lb)))
    return {"resident_bytes": b.value, "builds": n.value, "last_build_ms": round(ms.value, 3),
            "last_build_bytes": lb.value}


def dataProcessing() -> None:
    """dataProcessing, K:1735-1796: flexible-block pre-pass with 6-voxel blocks."""
    _lib.load().dataProcessing()
    check_last()


# ---------------------------------------------------------------- extensions

def init_distribution(bins, nbins: Optional[int] = None, dims=None, adopt: bool = False):
    """Make a distribution volume resident.

    bins: numpy array (nz, ny, nx, B) -> copied from host; or a torch CUDA tensor
    of the same shape -> copied device-to-device (adopt=False) or used in place
    (adopt=True, the caller keeps it alive).

    A numpy.float16 array or a torch.float16 CUDA tensor becomes resident as an
    f16 volume (half the bytes per voxel, B in 1, 2, 4, 8, 16, 32; volume_dtype()
    == "f16"); it renders bit-identically to the same records widened to
    float32.  Every other input is taken as float32, as before."""
    L = _lib.load()
    if hasattr(bins, "data_ptr") and getattr(bins, "is_cuda", False):
        shp = tuple(bins.shape)
        if dims is None:
            nz, ny, nx, nb = shp
            dims = (nx, ny, nz)
        nb = nbins if nbins is not None else shp[-1]
        init = (L.vr_init_distribution_f16 if str(bins.dtype) == "torch.float16"
                else L.vr_init_distribution)
        check(init(_ptr(bins), _extent(dims), int(nb), 2 if adopt else 1))
        return
    half = isinstance(bins, np.ndarray) and bins.dtype == np.float16
    a = np.ascontiguousarray(np.asarray(bins, dtype=np.float16 if half else np.float32))
    if dims is None:
        nz, ny, nx, nb = a.shape
        dims = (nx, ny, nz)
    nb = nbins if nbins is not None else a.shape[-1]
    init = L.vr_init_distribution_f16 if half else L.vr_init_distribution
    check(init(a.ctypes.data, _extent(dims), int(nb), 0))


def convert_f16() -> None:
    """Narrow the resident float32 record volume to f16 on the device (round to
    nearest even, subnormals kept); baked planes and layout copies are dropped.
    synthesize() then convert_f16() makes a large synthetic f16 volume."""
    check(_lib.load().vr_convert_f16())


def volume_dtype() -> str:
    """"f32" or "f16": the element type of the resident record volume."""
    return "f16" if check(_lib.load().vr_volume_dtype()) == _lib.VR_DTYPE_F16 else "f32"


def synthesize_codec(dims, nbins: int, ntemplates: int = 64, slots: int = 4,
                     seed: int = 20261015) -> None:
    """Generate the seeded synthetic codec volume (methods 4/5/6) directly in HBM."""
    check(_lib.load().vr_synthesize_codec(_extent(dims), int(nbins), int(ntemplates), int(slots),
                                          int(seed)))


def codec_info():
    """((X, Y, Z), nbins, ntemplates, slots, codebook_ptr, templates_ptr, errors_ptr)"""
    e = Extent()
    nb, nt, sl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cb, tp, er = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    check(_lib.load().vr_codec_info(ctypes.byref(e), ctypes.byref(nb), ctypes.byref(nt),
                                    ctypes.byref(sl), ctypes.byref(cb), ctypes.byref(tp),
                                    ctypes.byref(er)))
    return ((e.width, e.height, e.depth), nb.value, nt.value, sl.value, cb.value, tp.value,
            er.value)


def synthesize(dims, nbins: int, seed: int = 20261015) -> None:
    """Generate the seeded synthetic distribution volume directly in HBM."""
    check(_lib.load().vr_synthesize(_extent(dims), int(nbins), int(seed)))


def volume_info():
    e = Extent()
    nb = ctypes.c_int()
    p = ctypes.c_void_p()
    check(_lib.load().vr_volume_info(ctypes.byref(e), ctypes.byref(nb), ctypes.byref(p)))
    return (e.width, e.height, e.depth), nb.value, p.value


def volume_layout():
    """(row_pitch, slice_pitch) of the resident volume, in records."""
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    check(_lib.load().vr_volume_layout(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def set_stream(stream) -> None:
    """Stream for subsequent launches: a torch.cuda.Stream, a raw hipStream_t, or None."""
    raw = 0 if stream is None else (stream.cuda_stream if hasattr(stream, "cuda_stream")
                                    else int(stream))
    check(_lib.load().vr_set_stream(raw))


def set_tuning(key: str, value=None) -> None:
    """Set (value not None) or remove a tuning knob (include/vr.h vr_set_tuning):
    kernel-path overrides and occupancy caps for tests and tools.  Knobs change
    which kernel computes a frame, never its pixels; the library reads no
    environment variables."""
    L = _lib.load()
    check(L.vr_set_tuning(str(key).encode(), None if value is None else str(value).encode()))


def clear_tuning() -> None:
    """Remove every tuning knob (back to the default dispatch)."""
    _lib.load().vr_clear_tuning()


def make_desc(d_output, width: int, height: int, inv_view, density=0.05, brightness=1.0,
              transfer_offset=0.0, transfer_scale=1.0, query_method=1, volume_size=None,
              d_output_f=None, d_steps=None, d_tile_list=None, n_tiles=0) -> RenderDesc:
    d = RenderDesc()
    d.d_output = _ptr(d_output)
    d.d_output_f = _ptr(d_output_f)
    d.d_steps = _ptr(d_steps)
    d.width, d.height = int(width), int(height)
    m = np.asarray(inv_view, dtype=np.float32).reshape(12)
    for i in range(12):
        d.inv_view[i] = float(m[i])
    d.density, d.brightness = float(density), float(brightness)
    d.transfer_offset, d.transfer_scale = float(transfer_offset), float(transfer_scale)
    d.query_method = int(query_method)
    if volume_size is None:  # method 7's grid defaults to the resident volume's dims
        try:
            volume_size = volume_info()[0]
        except VRError:
            _lib.load().vr_clear_error()
            volume_size = codec_info()[0]
    d.volume_size = _extent(volume_size)
    d.d_tile_list = _ptr(d_tile_list)
    d.n_tiles = int(n_tiles)
    return d


def render(desc: RenderDesc) -> None:
    """Launch the march for an explicit descriptor (asynchronous)."""
    check(_lib.load().vr_render(ctypes.byref(desc)))


def count_footprint(desc: RenderDesc) -> int:
    """U: distinct records under all trilinear footprints (synchronous)."""
    return int(check(_lib.load().vr_count_footprint(ctypes.byref(desc))))


def footprint_bytes(desc: RenderDesc) -> int:
    """algorithmic volume bytes of one launch (methods 1-6; synchronous)"""
    return int(check(_lib.load().vr_footprint_bytes(ctypes.byref(desc))))


def unscatter_tiles(d_packed, d_tile_lists, n_ranks: int, n_slots: int, d_frame, width: int,
                    height: int) -> None:
    check(_lib.load().vr_unscatter_tiles(_ptr(d_packed), _ptr(d_tile_lists), int(n_ranks),
                                         int(n_slots), _ptr(d_frame), int(width), int(height)))


def last_kernel() -> str:
    """The march kernel (and its template arguments) the last render launched."""
    return _lib.load().vr_last_kernel().decode()


def stream_read(reps: int = 5):
    """Measured read ceiling: the resident record volume streamed by a coalesced
    16-B-per-lane read kernel (vr_stream_read).  Returns (bytes per pass,
    fastest ms, mean ms)."""
    ms = (ctypes.c_float * 2)()
    nbytes = ctypes.c_uint64(0)
    check(_lib.load().vr_stream_read(int(reps), ms, ctypes.byref(nbytes)))
    return int(nbytes.value), float(ms[0]), float(ms[1])


def debug_wave_clock(d_buf) -> None:
    """Tooling: per-wave {start, end, __smid} clocks of the pipelined, quad and
    ray-segmented marches into a device uint64 buffer of 48 * n_slots values
    (include/vr.h: up to 16 waves of 3 words per launch slot; None = off)."""
    check(_lib.load().vr_debug_wave_clock(None if d_buf is None else _ptr(d_buf)))


# ------------------------------------------- GMM volumes (config 5)

def init_gmm(wm, sigma, dims=None, z_base: int = 0, adopt: bool = False) -> None:
    """Make a K-component GMM volume resident.

    wm: (nzs, ny, nx, K, 2) float32 (w, mu) pairs; sigma: (nzs, ny, nx, K).  numpy
    arrays are copied from the host, torch CUDA tensors device-to-device (or used
    in place with adopt=True).  dims: the whole volume's (X, Y, Z) when only the
    slices [z_base, z_base + nzs) are given (default: wm's own shape).

    numpy.float16 arrays or torch.float16 CUDA tensors become resident as an f16
    volume (half the bytes, gmm_dtype() == "f16"), which
    renders bit-identically to the same records widened to float32; both planes
    must then be float16 (ValueError otherwise; an adopted f16 wm must be 16-byte
    aligned, sigma 8-byte).  Every other input is taken as float32, as before."""
    L = _lib.load()
    on_device = hasattr(wm, "data_ptr") and getattr(wm, "is_cuda", False)
    if on_device:
        half = str(wm.dtype) == "torch.float16"
    else:
        is_h = [isinstance(a, np.ndarray) and a.dtype == np.float16 for a in (wm, sigma)]
        if is_h[0] != is_h[1]:
            raise ValueError("wm and sigma must have the same dtype (both float16 or both float32)")
        half = is_h[0]
        # lists and other array-likes, as np.asarray takes them
        wm = np.asarray(wm, dtype=np.float16 if half else np.float32)
        sigma = np.asarray(sigma, dtype=np.float16 if half else np.float32)
    init = L.vr_init_gmm_f16 if half else L.vr_init_gmm
    if len(wm.shape) != 5 or int(wm.shape[4]) != 2:
        raise ValueError(f"wm must have shape (nzs, ny, nx, K, 2), got {tuple(wm.shape)}")
    nzs, ny, nx, K = (int(v) for v in wm.shape[:4])
    if dims is None:
        dims = (nx, ny, nzs)
    if tuple(int(v) for v in sigma.shape) != (nzs, ny, nx, K):
        raise ValueError(f"sigma must have shape wm.shape[:4] = {(nzs, ny, nx, K)}, "
                         f"got {tuple(sigma.shape)}")
    if on_device:
        import torch
        for name, t in (("wm", wm), ("sigma", sigma)):
            if not getattr(t, "is_cuda", False):
                raise ValueError(f"{name} must be a CUDA tensor like wm")
            if t.device != wm.device:
                raise ValueError(f"{name} is on {t.device}, wm on {wm.device}: both must be on "
                                 "the library's device")
            if t.dtype != wm.dtype:
                raise ValueError(f"wm and sigma must have the same dtype, got {wm.dtype} and "
                                 f"{sigma.dtype}")
            if t.dtype not in (torch.float32, torch.float16):
                raise ValueError(f"{name} must be float32 or float16, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous (the march reads dense planes)")
        check(init(_ptr(wm), _ptr(sigma), _extent(dims), K, int(z_base), nzs, 2 if adopt else 1))
        return
    a = np.ascontiguousarray(wm)
    b = np.ascontiguousarray(sigma)
    check(init(a.ctypes.data, b.ctypes.data, _extent(dims), K, int(z_base), nzs, 0))


def synthesize_gmm(dims, ncomp: int = 16, seed: int = 20261015, z_base: int = 0,
                   nslices: Optional[int] = None, dtype: str = "f32") -> None:
    """Generate slices [z_base, z_base + nslices) of the seeded synthetic GMM volume in HBM.
    dtype "f16": the same values rounded to nearest even, stored as halves."""
    if dtype not in ("f32", "f16"):
        raise ValueError(f'dtype must be "f32" or "f16", got {dtype!r}')
    if nslices is None:
        nslices = int(tuple(dims)[2]) - int(z_base)
    L = _lib.load()
    synth = L.vr_synthesize_gmm_f16 if dtype == "f16" else L.vr_synthesize_gmm
    check(synth(_extent(dims), int(ncomp), int(seed), int(z_base), int(nslices)))


def convert_gmm_f16() -> None:
    """Narrow the selected slot's resident float32 GMM planes to f16 on the device
    (round to nearest even, subnormals kept)."""
    check(_lib.load().vr_convert_gmm_f16())


def gmm_dtype() -> str:
    """"f32" or "f16": the element type of the selected slot's GMM volume."""
    return "f16" if check(_lib.load().vr_gmm_dtype()) == _lib.VR_DTYPE_F16 else "f32"


def gmm_info():
    """((X, Y, Z), K, z_base, nslices, wm_ptr, sigma_ptr) of the resident GMM volume
    (an f16 volume's pointers address halves)"""
    e = Extent()
    k, zb, ns = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    check(_lib.load().vr_gmm_info(ctypes.byref(e), ctypes.byref(k), ctypes.byref(zb),
                                  ctypes.byref(ns), ctypes.byref(a), ctypes.byref(b)))
    return (e.width, e.height, e.depth), k.value, zb.value, ns.value, a.value, b.value


def free_gmm() -> None:
    check(_lib.load().vr_free_gmm())


def gmm_select(slot: int) -> None:
    """Select GMM slot 0 or 1 (include/vr.h vr_gmm_select): the GMM calls act on it"""
    check(_lib.load().vr_gmm_select(int(slot)))


def gmm_slab(z_lo: int, z_hi: int, d_rays_out, d_n_rays_out, d_rays_in=None,
             n_rays_in: int = 0) -> _lib.GmmSlab:
    s = _lib.GmmSlab()
    s.z_lo, s.z_hi = int(z_lo), int(z_hi)
    s.d_rays_in = _ptr(d_rays_in) or None
    s.n_rays_in = int(n_rays_in)
    s.d_rays_out = _ptr(d_rays_out) or None
    s.d_n_rays_out = _ptr(d_n_rays_out) or None
    return s


def render_gmm(desc: RenderDesc, slab: Optional[_lib.GmmSlab] = None) -> None:
    """Launch the GMM march: the whole frame (slab None) or one slab of a chain.
    Query methods 1 (mean), 2 (variance), 10 (range probability, set_gmm_range) and
    11 (quantile, set_quantile / set_quantile_spread)."""
    L = _lib.load()
    check(L.vr_render_gmm(ctypes.byref(desc), None if slab is None else ctypes.byref(slab)))


def gmm_count_footprint(desc: RenderDesc, slab: Optional[_lib.GmmSlab] = None) -> int:
    """U of a whole-volume GMM render, or of one slab of a chain (synchronous)"""
    L = _lib.load()
    if slab is None:
        return int(check(L.vr_gmm_count_footprint(ctypes.byref(desc))))
    return int(check(L.vr_gmm_count_footprint_slab(ctypes.byref(desc), ctypes.byref(slab))))


# ------------------------------------- baked GMM statistics

def bake_gmm_stats() -> None:
    """Decode the selected slot's resident slices once per voxel into the library's
    two whole-volume GMM planes (mean, 16 x variance; include/vr.h
    vr_bake_gmm_stats), queued on the library stream.  The first call allocates
    the planes; they belong to no slot and outlive the records, so a volume is
    baked slab by slab (init_gmm / bake_gmm_stats / free_gmm per slab).  Records
    that change need release_gmm_stats() before they are baked again."""
    check(_lib.load().vr_bake_gmm_stats())


def release_gmm_stats() -> None:
    """Free the baked GMM planes."""
    check(_lib.load().vr_release_gmm_stats())


def gmm_stats_info():
    """((X, Y, Z), planes_ptr, plane_floats, slices_baked) of the baked GMM planes;
    planes_ptr None = no planes.  Plane 1 (16 x variance) follows plane 0 (mean)
    at planes_ptr + 4 * plane_floats bytes."""
    e = Extent()
    p, n, k = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    check(_lib.load().vr_gmm_stats_info(ctypes.byref(e), ctypes.byref(p), ctypes.byref(n),
                                        ctypes.byref(k)))
    return (e.width, e.height, e.depth), p.value, n.value, k.value


def render_gmm_baked(desc: RenderDesc) -> None:
    """A whole frame of query method 1 / 2 from the baked GMM planes (asynchronous),
    of method 10 from the range plane (bake_gmm_range) or of method 11 from the
    quantile plane (bake_gmm_quantile): bit-identical to render_gmm, with the plane
    march of render().  Takes tile lists, d_output_f and d_steps like render();
    every slice must be baked."""
    check(_lib.load().vr_render_gmm_baked(ctypes.byref(desc)))


# --------------------------------- weighted-bin query (method 10)

QUERY_WEIGHTED = _lib.VR_QUERY_WEIGHTED


def range_weights(lo: float, hi: float, n: int) -> np.ndarray:
    """The bin weights of the range probability P(lo <= v < hi) on the normalised
    value axis [0, 1], bin i covering [i / n, (i + 1) / n):
    w_i = n * max(0, min(hi, (i + 1) / n) - max(lo, i / n)) in float64, rounded to
    float32 -- vr_set_query_range's formula restated (a pure function: no library
    is loaded).  The bounds are first rounded to float32, as the C call takes them."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        raise ValueError("bounds must be finite with lo <= hi")
    i = np.arange(n, dtype=np.float64)
    a = np.maximum(lo, i / np.float64(n))
    b = np.minimum(hi, (i + 1.0) / np.float64(n))
    return (np.float64(n) * np.maximum(0.0, b - a)).astype(np.float32)


def set_bin_weights(w) -> None:
    """Set the weights of query method 10, s = sum w_i p_i (1, 2, 4, 8, 16 or 32
    finite floats, one per bin of the record volume); None clears them.  Host
    state only; a baked weighted plane is dropped."""
    L = _lib.load()
    if w is None:
        check(L.vr_set_bin_weights(None, 0))
        return
    a = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1))
    check(L.vr_set_bin_weights(a.ctypes.data, int(a.size)))


def bin_weights() -> np.ndarray:
    """The weights set (float32 array); VRError (VR_ERR_STATE) if none are."""
    w = np.zeros(32, np.float32)
    n = ctypes.c_int()
    check(_lib.load().vr_bin_weights(w.ctypes.data, ctypes.addressof(n)))
    return w[:n.value].copy()


def set_query_range(lo: float, hi: float, n: int) -> None:
    """Set the weights of the range probability P(lo <= v < hi) for n-bin records
    (vr_set_query_range; range_weights(lo, hi, n) gives the same floats)."""
    check(_lib.load().vr_set_query_range(float(lo), float(hi), int(n)))


def bake_weighted() -> None:
    """Decode the weighted statistic of every voxel once into a float plane
    (vr_bake_weighted, synchronous); method-10 frames then read the plane,
    bit-identical to the per-step frames, until the weights or the volume change."""
    check(_lib.load().vr_bake_weighted())


def release_weighted() -> None:
    """Drop the baked weighted plane: method 10 decodes the records per step again."""
    check(_lib.load().vr_release_weighted())


def weighted_info():
    """(plane_ptr, plane_floats) of the baked weighted plane; plane_ptr None = not baked"""
    p, n = ctypes.c_void_p(), ctypes.c_uint64()
    check(_lib.load().vr_weighted_info(ctypes.addressof(p), ctypes.addressof(n)))
    return p.value, n.value


# --------------------------------- quantile query (method 11)

QUERY_QUANTILE = _lib.VR_QUERY_QUANTILE


def set_quantile(q) -> None:
    """Set query method 11 to the quantile Q(q), the value on the normalised axis
    [0, 1] where a voxel's CDF reaches q (0.5: the median); None clears it.  Host
    state only; a baked quantile plane is dropped."""
    L = _lib.load()
    check(L.vr_clear_quantile() if q is None else L.vr_set_quantile(float(q)))


def set_quantile_spread(lo: float, hi: float) -> None:
    """Set query method 11 to the spread Q(hi) - Q(lo) (0.25, 0.75: the
    interquartile range); 0 <= lo <= hi <= 1."""
    check(_lib.load().vr_set_quantile_spread(float(lo), float(hi)))


def quantile():
    """(q_lo, q_hi, spread) as set (a single quantile: q_lo == q_hi, spread False);
    VRError (VR_ERR_STATE) if none is."""
    lo, hi, sp = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
    check(_lib.load().vr_quantile(ctypes.addressof(lo), ctypes.addressof(hi),
                                  ctypes.addressof(sp)))
    return lo.value, hi.value, bool(sp.value)


def bake_quantile() -> None:
    """Decode the quantile statistic of every voxel once into a float plane
    (vr_bake_quantile, synchronous); method-11 frames then read the plane,
    bit-identical to the per-step frames, until the quantile or the volume change."""
    check(_lib.load().vr_bake_quantile())


def release_quantile() -> None:
    """Drop the baked quantile plane: method 11 decodes the records per step again."""
    check(_lib.load().vr_release_quantile())


def quantile_info():
    """(plane_ptr, plane_floats) of the baked quantile plane; plane_ptr None = not baked"""
    p, n = ctypes.c_void_p(), ctypes.c_uint64()
    check(_lib.load().vr_quantile_info(ctypes.addressof(p), ctypes.addressof(n)))
    return p.value, n.value


# ---------------------- distribution-distance query (method 12)

QUERY_DISTANCE = _lib.VR_QUERY_DISTANCE
_DIST_METRICS = {"l1": _lib.VR_DIST_L1, "emd": _lib.VR_DIST_EMD, "ks": _lib.VR_DIST_KS}


def _dist_metric(metric) -> int:
    if isinstance(metric, str):
        if metric.lower() not in _DIST_METRICS:
            raise ValueError(f"metric must be one of {sorted(_DIST_METRICS)}, got {metric!r}")
        return _DIST_METRICS[metric.lower()]
    return int(metric)


def set_query_target(h, metric="l1", similarity=False) -> None:
    """Set the target record of query method 12, the distance D(p, h) of every
    voxel's record p from h (1, 2, 4, 8, 16 or 32 finite floats, one per bin of the
    record volume) under metric "l1" (total variation), "emd" (earth mover's on the
    value axis [0, 1]) or "ks" (largest CDF gap); similarity: frames of 1 - D.
    None clears it.  Host state only; a baked distance plane is dropped."""
    L = _lib.load()
    if h is None:
        check(L.vr_set_query_target(None, 0, 0, 0))
        return
    a = np.ascontiguousarray(np.asarray(h, dtype=np.float32).reshape(-1))
    check(L.vr_set_query_target(a.ctypes.data, int(a.size), _dist_metric(metric),
                                int(bool(similarity))))


def query_target():
    """(h, metric, similarity) as set: the target (float32 array), the metric's
    name and the flag; VRError (VR_ERR_STATE) if nothing is set."""
    h = np.zeros(32, np.float32)
    n, m, s = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(_lib.load().vr_query_target(h.ctypes.data, ctypes.addressof(n), ctypes.addressof(m),
                                      ctypes.addressof(s)))
    name = {v: k for k, v in _DIST_METRICS.items()}[m.value]
    return h[:n.value].copy(), name, bool(s.value)


def set_query_target_region(lo, hi, metric="l1", similarity=False) -> None:
    """Query by example: the target becomes the mean record of the box
    [lo, hi) = [x0, x1) x [y0, y1) x [z0, z1) of the resident record volume (at most
    4096 voxels; vr_set_query_target_region).  query_target() reads it back."""
    x0, y0, z0 = (int(v) for v in lo)
    x1, y1, z1 = (int(v) for v in hi)
    check(_lib.load().vr_set_query_target_region(x0, y0, z0, x1, y1, z1, _dist_metric(metric),
                                                 int(bool(similarity))))


def bake_distance() -> None:
    """Decode the distance statistic of every voxel once into a float plane
    (vr_bake_distance, synchronous); method-12 frames then read the plane,
    bit-identical to the per-step frames, until the target or the volume change."""
    check(_lib.load().vr_bake_distance())


def release_distance() -> None:
    """Drop the baked distance plane: method 12 decodes the records per step again."""
    check(_lib.load().vr_release_distance())


def distance_info():
    """(plane_ptr, plane_floats) of the baked distance plane; plane_ptr None = not baked"""
    p, n = ctypes.c_void_p(), ctypes.c_uint64()
    check(_lib.load().vr_distance_info(ctypes.addressof(p), ctypes.addressof(n)))
    return p.value, n.value


# ---------------------------- level-crossing query (method 13)

QUERY_CROSSING = _lib.VR_QUERY_CROSSING


def set_crossing_weights(w) -> None:
    """Set the weights of query method 13: F = sum w_i p_i is the per-voxel
    probability whose level-crossing probability 1 - prod F_c - prod (1 - F_c) over a
    cell's 8 corners (taken as independent) the frame shows (1, 2, 4, 8, 16 or 32
    finite floats, one per bin of the record volume); None clears them.  Host state
    only, apart from method 10's weights; a baked crossing plane is dropped."""
    L = _lib.load()
    if w is None:
        check(L.vr_set_crossing_weights(None, 0))
        return
    a = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1))
    check(L.vr_set_crossing_weights(a.ctypes.data, int(a.size)))


def crossing_weights() -> np.ndarray:
    """The crossing weights set (float32 array); VRError (VR_ERR_STATE) if none are."""
    w = np.zeros(32, np.float32)
    n = ctypes.c_int()
    check(_lib.load().vr_crossing_weights(w.ctypes.data, ctypes.addressof(n)))
    return w[:n.value].copy()


def set_isovalue(theta: float, n: int) -> None:
    """Set the crossing weights to the CDF at the isovalue theta for n-bin records:
    F = P(v < theta) on the normalised value axis [0, 1] (vr_set_isovalue; the floats
    of range_weights(0, theta, n))."""
    check(_lib.load().vr_set_isovalue(float(theta), int(n)))


def bake_crossing() -> None:
    """Decode F of every voxel once into a float plane (vr_bake_crossing,
    synchronous); method-13 frames then read the plane, bit-identical to the
    per-step frames, until the crossing weights or the volume change."""
    check(_lib.load().vr_bake_crossing())


def release_crossing() -> None:
    """Drop the baked crossing plane: method 13 decodes the records per step again."""
    check(_lib.load().vr_release_crossing())


def crossing_info():
    """(plane_ptr, plane_floats) of the baked crossing plane; plane_ptr None = not baked"""
    p, n = ctypes.c_void_p(), ctypes.c_uint64()
    check(_lib.load().vr_crossing_info(ctypes.addressof(p), ctypes.addressof(n)))
    return p.value, n.value


# ------------------- range probability of GMM volumes (method 10)

def set_gmm_range(lo: float, hi: float) -> None:
    """Set query method 10 on GMM volumes to P(lo <= v < hi) of a voxel's mixture;
    lo = -inf gives the CDF at hi, hi = +inf the exceedance of lo.  Host state
    only; the baked range plane is dropped."""
    check(_lib.load().vr_set_gmm_range(float(lo), float(hi)))


def clear_gmm_range() -> None:
    """No range set; the baked range plane is dropped."""
    check(_lib.load().vr_clear_gmm_range())


def gmm_range():
    """(lo, hi) as set (float32 values); VRError (VR_ERR_STATE) if none is."""
    lo, hi = ctypes.c_float(), ctypes.c_float()
    check(_lib.load().vr_gmm_range(ctypes.addressof(lo), ctypes.addressof(hi)))
    return lo.value, hi.value


def gmm_phi_table():
    """(c (4, nseg + 1) float32, nseg, h, zmax): the table of E = Phi - 1/2 the
    range-probability kernels read (vr_gmm_phi_table), c[j][i] the coefficient
    of t^j in segment i; a read-only copy."""
    p, n = ctypes.c_void_p(), ctypes.c_int()
    h, zmax = ctypes.c_float(), ctypes.c_float()
    check(_lib.load().vr_gmm_phi_table(ctypes.addressof(p), ctypes.addressof(n),
                                       ctypes.addressof(h), ctypes.addressof(zmax)))
    rows = n.value + 1
    c = np.ctypeslib.as_array(ctypes.cast(p.value, ctypes.POINTER(ctypes.c_float)),
                              shape=(4, rows)).copy()
    c.setflags(write=False)
    return c, n.value, h.value, zmax.value


def bake_gmm_range() -> None:
    """Decode the range probability of the selected slot's resident slices once per
    voxel into the library's whole-volume range plane (vr_bake_gmm_range), queued
    on the library stream.  A plane of its own beside the bake_gmm_stats planes,
    baked slab by slab like them; render_gmm_baked with query method 10 reads it.
    Records that change need release_gmm_range() before they are baked again."""
    check(_lib.load().vr_bake_gmm_range())


def release_gmm_range() -> None:
    """Free the baked range plane (the range stays set)."""
    check(_lib.load().vr_release_gmm_range())


def gmm_range_info():
    """((X, Y, Z), plane_ptr, plane_floats, slices_baked) of the baked range plane;
    plane_ptr None = no plane."""
    e = Extent()
    p, n, k = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    check(_lib.load().vr_gmm_range_info(ctypes.byref(e), ctypes.byref(p), ctypes.byref(n),
                                        ctypes.byref(k)))
    return (e.width, e.height, e.depth), p.value, n.value, k.value


# ------------------------- quantile of GMM volumes (method 11)
# (the quantile itself: set_quantile / set_quantile_spread / quantile above)

def gmm_quantile_steps() -> int:
    """The bisection steps N of the GMM quantile search (vr_gmm_quantile_steps)."""
    return int(_lib.load().vr_gmm_quantile_steps())


def bake_gmm_quantile() -> None:
    """Decode the quantile (or the spread) that is set of the selected slot's resident
    slices once per voxel into the library's whole-volume quantile plane
    (vr_bake_gmm_quantile), queued on the library stream.  A plane of its own beside
    the bake_gmm_stats and bake_gmm_range planes, baked slab by slab like them;
    render_gmm_baked with query method 11 reads it.  Any set_quantile /
    set_quantile_spread drops it.  Records that change need release_gmm_quantile()
    before they are baked again."""
    check(_lib.load().vr_bake_gmm_quantile())


def release_gmm_quantile() -> None:
    """Free the baked GMM quantile plane (the quantile stays set)."""
    check(_lib.load().vr_release_gmm_quantile())


def gmm_quantile_info():
    """((X, Y, Z), plane_ptr, plane_floats, slices_baked) of the baked GMM quantile
    plane; plane_ptr None = no plane."""
    e = Extent()
    p, n, k = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    check(_lib.load().vr_gmm_quantile_info(ctypes.byref(e), ctypes.byref(p), ctypes.byref(n),
                                           ctypes.byref(k)))
    return (e.width, e.height, e.depth), p.value, n.value, k.value


# ------------------- user-defined transfer function

TF_MAX = _lib.VR_TF_MAX

# the built-in table: the reference's nine RGBA entries (K:2323-2326).  Set as a
# custom table it gives the built-in frames bit for bit.
REFERENCE_TF = np.array([
    [0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 1.0], [1.0, 0.5, 0.0, 1.0], [1.0, 1.0, 0.0, 1.0],
    [0.0, 1.0, 0.0, 1.0], [0.0, 1.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0], [1.0, 0.0, 1.0, 1.0],
    [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
REFERENCE_TF.setflags(write=False)


def set_transfer_function(table) -> None:
    """Classify frames through `table`, (n, 4) finite floats r, g, b, a with
    1 <= n <= TF_MAX, sampled as the built-in nine entries are (linear, clamped,
    8-bit weights; values not clamped); None returns to the built-in table.  Host
    state only, the caller's like the bin weights: it survives new volumes and
    freeCudaBuffers and drops no baked plane.  While a table is set frames come from
    baked planes (bake_stats, bake_weighted / _quantile / _distance / _crossing,
    render_gmm_baked); everything else raises VRError (VR_ERR_UNSUPPORTED)."""
    L = _lib.load()
    if table is None:
        check(L.vr_set_transfer_function(None, 0))
        return
    a = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"a transfer function is (n, 4) RGBA entries, got shape {a.shape}")
    check(L.vr_set_transfer_function(a.ctypes.data, int(a.shape[0])))


def transfer_function():
    """The table set, an (n, 4) float32 array; None: the built-in table is in use."""
    t = np.zeros((TF_MAX, 4), np.float32)
    n = ctypes.c_int()
    check(_lib.load().vr_transfer_function(t.ctypes.data, ctypes.addressof(n)))
    return t[:n.value].copy() if n.value else None


# ------------- 2-D transfer function over two planes

TF2_MAX = _lib.VR_TF2_MAX


def set_transfer_function_2d(table, method_v=None, v_offset: float = 0.0,
                             v_scale: float = 1.0) -> None:
    """Classify frames through `table`, (nv, nu, 4) finite floats r, g, b, a with
    1 <= nu, nv <= 256 and nu * nv <= TF2_MAX, looked up bilinearly at
    ((su - transfer_offset) * transfer_scale, (sv - v_offset) * v_scale): su the
    sample of the frame's query_method's plane, sv that of method_v's plane, both
    from one footprint.  None clears it (the other arguments are not read).  Host
    state of the caller's, kept as set_transfer_function's is; setting one of the
    two tables clears the other.  While it is set frames come from two resident
    baked planes of one family (1/2/3/10-13, or the codec's 4/5/6; render_gmm_baked:
    1, 2, 10, 11, 13); everything else raises VRError (VR_ERR_UNSUPPORTED)."""
    L = _lib.load()
    if table is None:
        check(L.vr_set_transfer_function_2d(None, 0, 0, 0, 0.0, 1.0))
        return
    a = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"a 2-D transfer function is (nv, nu, 4) RGBA entries, got shape {a.shape}")
    if method_v is None:
        raise ValueError("method_v: the query method whose plane is the table's v axis")
    check(L.vr_set_transfer_function_2d(a.ctypes.data, int(a.shape[1]), int(a.shape[0]),
                                        int(method_v), float(v_offset), float(v_scale)))


def transfer_function_2d():
    """(table (nv, nu, 4) float32, method_v, v_offset, v_scale) of the 2-D table set;
    None: none is set."""
    t = np.zeros(4 * TF2_MAX, np.float32)
    nu, nv, mv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    off, scale = ctypes.c_float(), ctypes.c_float()
    check(_lib.load().vr_transfer_function_2d(
        t.ctypes.data, ctypes.addressof(nu), ctypes.addressof(nv), ctypes.addressof(mv),
        ctypes.addressof(off), ctypes.addressof(scale)))
    if not nu.value:
        return None
    return (t[:4 * nu.value * nv.value].reshape(nv.value, nu.value, 4).copy(), mv.value,
            off.value, scale.value)


# ------------------- ray projections of baked planes

PROJ_MAX, PROJ_MIN, PROJ_MEAN = _lib.VR_PROJ_MAX, _lib.VR_PROJ_MIN, _lib.VR_PROJ_MEAN
_PROJ_NAMES = {None: 0, "max": PROJ_MAX, "min": PROJ_MIN, "mean": PROJ_MEAN}


def set_projection(mode) -> None:
    """What is done with the samples along a ray: "max", "min" or "mean" (or PROJ_MAX
    / PROJ_MIN / PROJ_MEAN) reduces every ray's samples to that one value -- no opacity
    test, no early end -- and classifies it once, through the table of
    set_transfer_function if one is set, else the built-in one; None (or 0) returns to
    compositing.  Host state only, the caller's like the table: it survives new
    volumes and freeCudaBuffers.  While a projection is set frames come from baked
    planes, as under a 1-D table; everything else, and any frame while a 2-D table is
    set, raises VRError (VR_ERR_UNSUPPORTED)."""
    if mode is None or isinstance(mode, str):
        if mode not in _PROJ_NAMES:
            raise ValueError(f'a projection is "max", "min", "mean" or None, got {mode!r}')
        mode = _PROJ_NAMES[mode]
    check(_lib.load().vr_set_projection(int(mode)))


def projection():
    """The projection set: "max", "min" or "mean"; None: frames are composited."""
    m = _lib.load().vr_projection()
    return {v: k for k, v in _PROJ_NAMES.items()}[m]


# ------------------- headlight gradient shading

def set_light(ambient=0.3, diffuse=0.7, specular=0.0, shininess=1) -> None:
    """A light at the eye for frames from baked planes: every classified sample's
    colour becomes rgb * (ambient + diffuse * c) + specular * c ** shininess, c the
    cosine between the ray and the gradient of the plane inside the sample's cell
    (for method 13 the gradient of F, the normal of the probabilistic isosurface).
    shininess is a power of two from 1 to 128 (ValueError otherwise); the coefficients
    are finite and >= 0 (VRError otherwise).  set_light(None) turns the light off.
    Opacity is not lit, so rays keep their lengths; (1, 0, 0) is the unlit frame bit
    for bit.  Host state only, the caller's like the table: it survives new volumes
    and freeCudaBuffers.  While the light is on frames come from baked planes, as under
    a 1-D table; everything else, and any frame while a 2-D table or a projection is
    set, raises VRError (VR_ERR_UNSUPPORTED)."""
    L = _lib.load()
    if ambient is None:
        check(L.vr_set_light(None))
        return
    if (isinstance(shininess, bool) or not isinstance(shininess, (int, np.integer))
            or shininess < 1 or shininess > 128 or shininess & (shininess - 1)):
        raise ValueError(f"shininess is a power of two from 1 to 128, got {shininess!r}")
    light = _lib.Light(float(ambient), float(diffuse), float(specular),
                       int(shininess).bit_length() - 1)
    check(L.vr_set_light(ctypes.byref(light)))


def light():
    """The light set, as a dict of ambient, diffuse, specular and shininess; None: off."""
    out = _lib.Light()
    if not _lib.load().vr_light_state(ctypes.byref(out)):
        return None
    return {"ambient": out.ambient, "diffuse": out.diffuse, "specular": out.specular,
            "shininess": 1 << out.shininess_log2}


# ------------------- gradient-magnitude planes

GRADIENT = _lib.VR_QUERY_GRADIENT


def gradient_of(m: int) -> int:
    """The query method of the gradient-magnitude plane of source method m (1-6,
    10-13): GRADIENT + m.  Frames of it come from the plane bake_gradient(m) makes,
    wherever a baked plane is served: under a 1-D table, as the frame's method or as
    method_v of a 2-D table, under a projection, under the light, or with none of
    these through the built-in table."""
    m = int(m)
    if not (1 <= m <= 6 or 10 <= m <= 13):
        raise ValueError(f"method {m} has no baked plane to take the gradient of")
    return GRADIENT + m


def bake_gradient(m: int) -> None:
    """Bake |grad s| of the resident baked plane s of method m into a plane of its own
    (vr_bake_gradient, synchronous): central differences, one-sided on the volume's
    faces, per unit of the normalised coordinates.  VRError (VR_ERR_STATE) if m's plane
    is not baked.  The plane goes when its source's plane goes."""
    check(_lib.load().vr_bake_gradient(int(m)))


def release_gradient(m: int) -> None:
    """Drop the gradient plane of method m; m's own plane stays."""
    check(_lib.load().vr_release_gradient(int(m)))


def gradient_info(m: int):
    """(plane_ptr, plane_floats, max) of the gradient plane of method m, max the
    largest magnitude of the volume; (None, 0, 0.0) if it is not baked."""
    p, n, mx = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_float()
    check(_lib.load().vr_gradient_info(int(m), ctypes.addressof(p), ctypes.addressof(n),
                                       ctypes.addressof(mx)))
    return p.value, n.value, mx.value


# ------------------- value ranges and histograms of baked planes

HIST_MAX = _lib.VR_HIST_MAX


def _box(box):
    """box as six C ints (x0, x1, y0, y1, z0, z1), or None: the whole volume"""
    if box is None:
        return None
    b = [int(v) for v in np.asarray(box).ravel()]
    if len(b) != 6:
        raise ValueError("a box is (x0, x1, y0, y1, z0, z1)")
    return (ctypes.c_int * 6)(*b)


def plane_range(method: int, box=None):
    """(min, max, n_nan) of the resident baked plane of `method` (1-6, 10-13 or
    gradient_of(m)) over box = (x0, x1, y0, y1, z0, z1) in voxels, None: the whole
    volume (vr_plane_range, synchronous).  min and max are numpy.float32 over the voxels
    that are not NaN, -0 below +0; NaN if every voxel is NaN.  n_nan counts those."""
    lo, hi, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_uint64()
    b = _box(box)
    check(_lib.load().vr_plane_range(int(method), ctypes.addressof(b) if b else None,
                                     ctypes.addressof(lo), ctypes.addressof(hi),
                                     ctypes.addressof(n)))
    return np.float32(lo.value), np.float32(hi.value), n.value


def plane_window(method: int, box=None):
    """(offset, scale) that spreads the plane's values over a table: offset = min and
    scale = 1 / (max - min) in float32, 1.0 when max <= min, as transfer_offset /
    transfer_scale or v_offset / v_scale."""
    lo, hi, _ = plane_range(method, box)
    if not hi > lo:
        return float(lo), 1.0
    with np.errstate(all="ignore"):
        return float(lo), float(np.float32(1) / np.float32(hi - lo))


def plane_histogram(method_u: int, nu: int, window_u=None, method_v: Optional[int] = None,
                    nv: int = 1, window_v=None, box=None) -> np.ndarray:
    """The histogram of the resident plane of method_u over nu bins, or with method_v the
    joint histogram of the two planes over nv x nu bins, of the voxels of `box` (None:
    the whole volume): numpy.uint64 of shape (nv, nu), bin [j, i] the cell of entry
    (j, i) of the table a frame under the same windows uses (vr_plane_histogram,
    synchronous).  A window is (offset, scale); None: plane_window of that plane and
    box.  Values outside a window count in its edge bins, a NaN in bin 0."""
    wu = plane_window(method_u, box) if window_u is None else window_u
    wv = (0.0, 1.0)
    if method_v is not None:
        wv = plane_window(method_v, box) if window_v is None else window_v
    nu, nv = int(nu), int(nv)
    # (bin counts the library refuses reach it with one word to write nothing into)
    ok = nu >= 1 and nv >= 1 and nu * nv <= HIST_MAX
    counts = np.zeros((nv, nu) if ok else (1, 1), dtype=np.uint64)
    b = _box(box)
    check(_lib.load().vr_plane_histogram(
        int(method_u), float(wu[0]), float(wu[1]), int(nu),
        0 if method_v is None else int(method_v), float(wv[0]), float(wv[1]), int(nv),
        ctypes.addressof(b) if b else None, counts.ctypes.data))
    return counts


def plane_kernel_ms() -> float:
    """HIP-event time in ms of the kernel of the last plane_range / plane_histogram"""
    ms = ctypes.c_float()
    check(_lib.load().vr_plane_kernel_ms(ctypes.addressof(ms)))
    return ms.value


def version() -> str:
    return _lib.load().vr_version().decode()


__all__ = [
    "render_kernel", "copyInvViewMatrix", "initCuda", "freeCudaBuffers", "setTextureFilterMode",
    "basicDataProcessing", "dataProcessing", "init_distribution", "init_codec", "init_flex",
    "flex_process", "flex_info", "load_flex_files", "parse_flex_files", "synthesize", "synthesize_codec", "codec_info",
    "volume_info",
    "volume_layout",
    "set_stream", "set_tuning", "clear_tuning", "make_desc", "render", "count_footprint", "footprint_bytes", "unscatter_tiles", "last_kernel", "debug_wave_clock", "stream_read", "version",
    "init_gmm", "synthesize_gmm", "gmm_info", "free_gmm", "gmm_select", "gmm_slab", "render_gmm",
    "gmm_count_footprint", "bake_stats", "release_stats", "stats_info", "set_layout_budget",
    "layout_info", "convert_f16", "volume_dtype", "convert_gmm_f16", "gmm_dtype",
    "bake_gmm_stats", "release_gmm_stats", "gmm_stats_info", "render_gmm_baked",
    "QUERY_WEIGHTED", "range_weights", "set_bin_weights", "bin_weights", "set_query_range",
    "bake_weighted", "release_weighted", "weighted_info",
    "QUERY_QUANTILE", "set_quantile", "set_quantile_spread", "quantile", "bake_quantile",
    "release_quantile", "quantile_info",
    "QUERY_DISTANCE", "set_query_target", "query_target", "set_query_target_region",
    "bake_distance", "release_distance", "distance_info",
    "QUERY_CROSSING", "set_crossing_weights", "crossing_weights", "set_isovalue",
    "bake_crossing", "release_crossing", "crossing_info",
    "set_gmm_range", "clear_gmm_range", "gmm_range", "gmm_phi_table", "bake_gmm_range",
    "release_gmm_range", "gmm_range_info",
    "gmm_quantile_steps", "bake_gmm_quantile", "release_gmm_quantile", "gmm_quantile_info",
    "TF_MAX", "REFERENCE_TF", "set_transfer_function", "transfer_function",
    "TF2_MAX", "set_transfer_function_2d", "transfer_function_2d",
    "PROJ_MAX", "PROJ_MIN", "PROJ_MEAN", "set_projection", "projection",
    "set_light", "light",
    "GRADIENT", "gradient_of", "bake_gradient", "release_gradient", "gradient_info",
    "HIST_MAX", "plane_range", "plane_window", "plane_histogram", "plane_kernel_ms",
    "VRError", "PAD",
]
