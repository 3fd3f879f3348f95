"""Seeded random sessions and the host model they are held to (run on the GPU by
tests/test_gpu_sessions.py; the CPU census is tests/test_session_model.py).

No GPU and no library: numpy and the generators of random_cases only.

The other sweeps build the library up for one frame and tear it down again.  A session
keeps one process's library alive over 16-20 state-changing calls -- new contents of the
same shape and of others, rebakes, tables and lights that come and go, a second stream,
bad calls --
and after every call asks two questions: do the getters report what include/vr.h says
they must (Model.census), and does a frame rendered now come from the data and the state
that are current (Model.expect).  A plane, a copy or a table that outlives its cause
answers one of them wrong.

session(seed) is a plain dict: the flavour (seed % 4: records, records+codec, gmm,
mixed), the first volume and the ops.  Every op carries what the generator's own Model
made of it: `status` (0, or the status a bad call must be refused with), `probe` (a frame
the library must serve now, or None), `refuse` (a frame it must refuse now, with that
status, or None) and, one step in four or at the next one after it that has a record or
codec plane resident, `stat` (a plane_range or plane_histogram call on such a plane).  Ops are dealt in scenes -- make planes resident, then apply one
documented cause of their drop -- so that every (plane family, cause) pair of DROPS occurs
with the plane resident; inside the scenes the caller's state turns through SPRINKLES,
which sets every pair of light, projection and 2-D table against each other, and after
them comes the stream scene (a table used on one stream, the stream changed, the table set
anew: table_upload's drain across streams) and SPRINKLES_B (the layout budget, a knob).
Every second records session starts with the layout scene (the knob and the side view that
make an axis-rows copy, which a later op of the session must drop) and every second mixed
session uploads records of another shape over resident planes (the reshape scene).

Model restates include/vr.h; each rule stands next to the header sentence it restates
(quoted as vr.h: "..." with the entry point the sentence is documented at).  Where more
than one refusal applies to a frame -- a statistic with no state set under a table that
refuses what it has no plane for -- the answer is the first in the order of checks the
header states at vr_set_transfer_function, and the sessions deal such frames too.
"""
import copy
import math

import numpy as np

import random_cases as rc
import ref_weighted

OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -4
G = rc.GRADIENT
SOURCES = (1, 2, 3, 4, 5, 6, 10, 11, 12, 13)   # the methods with a baked plane (vr.h: VR_GRADIENT_OF)
QUERIES = (10, 11, 12, 13)
FLAVOURS = ("records", "records+codec", "gmm", "mixed")
N_SESSIONS = 48
FRAME_MAX = (64, 48)
GMM_SETS = {"stats": (1, 2), "range": (10, 13), "quant": (11,)}   # set -> the methods that read it
PROJECTIONS = ("max", "min", "mean")
KNOBS = (("VR_WG_PER_CU", "2"), ("VR_SEG_RAYS", "0"))   # (the second: tests/test_gpu_layout.py's)


def _f32(x):
    return float(np.float32(x))


def interval_weights(lo, hi, n):
    """vr.h (vr_set_query_range): "w_i = (float)(n * max(0, min(hi, (i + 1) / n) -
    max(lo, i / n))) evaluated in double", lo and hi the floats received"""
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    i = np.arange(n, dtype=np.float64)
    a, b = np.maximum(lo, i / np.float64(n)), np.minimum(hi, (i + 1.0) / np.float64(n))
    return (np.float64(n) * np.maximum(0.0, b - a)).astype(np.float32)


def weights_value(d):
    """the float32 weights of a weights descriptor (an op's argument, the model's state)"""
    if d is None:
        return None
    if d["kind"] == "seeded":
        return ref_weighted.seeded_weights(d["n"], seed=d["wseed"])
    return interval_weights(d["lo"], d["hi"], d["n"])   # "range", and "isovalue" with lo = 0


def table_value(spec, poison=False):
    t = rc.make_table({k: spec[k] for k in ("shape", "kind", "seed")})
    if poison:
        t = t.copy()
        t.reshape(-1)[1] = np.nan
    return t


def lin_bins(n):
    return n in rc.INSTANCE_BINS


def plane_family(m):
    """records or codec: whose grid the plane of method m (or gradient method 32 + m) has"""
    src = m - G if m > G else m
    if src in (1, 2, 3) or src in QUERIES:
        return "records"
    return "codec" if src in (4, 5, 6) else None


# The documented causes of each plane family's drop: family -> the ops that drop it.  The
# census (tests/test_session_model.py) asks that each pair occurs with the plane resident
# and that the model drops a plane on no other op.
_VOLUME = ("init_distribution", "convert_f16", "release_stats", "freeCudaBuffers")
DROPS = {
    # vr.h (vr_bake_stats): "Re-uploading or releasing a volume drops its planes";
    # (vr_convert_f16): "Baked planes and layout copies are dropped, as by a re-upload"
    "stats": _VOLUME,
    "cstats": ("init_codec", "release_stats", "freeCudaBuffers"),
    # vr.h (vr_bake_weighted): "The plane is dropped by any change of the weights, a new
    # upload or release of the volume, vr_convert_f16, vr_release_stats, freeCudaBuffers and
    # vr_release_weighted"
    "weighted": _VOLUME + ("set_bin_weights", "set_query_range", "clear_bin_weights",
                           "release_weighted"),
    # vr.h (vr_bake_quantile): "dropped by any call that sets or clears the quantile, ..."
    "quantile": _VOLUME + ("set_quantile", "set_quantile_spread", "clear_quantile",
                           "release_quantile"),
    # vr.h (vr_bake_distance): "dropped by any call that sets or clears the target, ..."
    "distance": _VOLUME + ("set_query_target", "set_query_target_region", "clear_query_target",
                           "release_distance"),
    # vr.h (vr_bake_crossing): "dropped by any call that sets or clears the crossing weights, ..."
    "crossing": _VOLUME + ("set_isovalue", "set_crossing_weights", "clear_crossing_weights",
                           "release_crossing"),
    # vr.h (vr_release_gmm_stats): "frees the planes (freeCudaBuffers does too)"
    "gmm stats": ("release_gmm_stats", "freeCudaBuffers"),
    # vr.h (vr_bake_gmm_range): "dropped by vr_set_gmm_range, vr_clear_gmm_range,
    # vr_release_gmm_range and freeCudaBuffers"
    "gmm range": ("set_gmm_range", "clear_gmm_range", "release_gmm_range", "freeCudaBuffers"),
    # vr.h (vr_bake_gmm_quantile): "dropped by vr_set_quantile, vr_set_quantile_spread,
    # vr_clear_quantile, vr_release_gmm_quantile and freeCudaBuffers"
    "gmm quant": ("set_quantile", "set_quantile_spread", "clear_quantile", "release_gmm_quantile",
                  "freeCudaBuffers"),
}
# vr.h (vr_bake_gradient): "Whatever frees or replaces a source's plane ... frees its
# gradient plane first"; "vr_release_gradient(m) frees the gradient plane alone"
for _m in SOURCES:
    DROPS[f"gradient {_m}"] = ("source went", "release_gradient")
QUERY_FAMILY = {10: "weighted", 11: "quantile", 12: "distance", 13: "crossing"}
QUERY_NAME = {10: "weighted", 11: "quantile", 12: "distance", 13: "crossing"}


class Model:
    """A host-side picture of the library: apply(op) -> status, census(), expect(probe).
    State is plain data (copy.deepcopy gives a snapshot)."""

    def __init__(self):
        # ---- the caller's state.  vr.h (vr_set_transfer_function): "The table is the
        # caller's, like the bin weights: it survives new volumes, vr_convert_f16,
        # vr_release_*, and freeCudaBuffers"; the same sentence stands at the 2-D table,
        # vr_set_projection and vr_set_light, and (vr_bake_crossing) "the weights are the
        # caller's and survive all of these except a call that sets or clears them"
        self.weights = None      # descriptor, weights_value()
        self.quant = None        # (q_lo, q_hi, spread)
        self.target = None       # dict(h=[floats], metric, similarity)
        self.xweights = None     # descriptor
        self.gmm_range = None    # (lo, hi)
        self.tf = None           # table spec
        self.tf2 = None          # dict(table=spec, mv, voff, vscale)
        self.proj = None
        self.light = None        # (ambient, diffuse, specular, shininess_log2)
        self.stream = 0
        self.budget = None
        self.knobs = {}
        # ---- what is resident
        self.vol = None          # record volume spec: dims, nb, dtype, seed, narrowed, adopt
        self.codec = None        # codec volume spec: dims, nb, seed
        self.stats = False
        self.cstats = False
        self.qplane = {m: False for m in QUERIES}
        self.grad = {m: False for m in SOURCES}
        self.gmm = [None, None]  # per slot: dict(spec=dims, K, dtype, seed, narrowed; z_base, nzs)
        self.slot = 0
        self.gplanes = {k: None for k in GMM_SETS}   # dict(dims, src=[spec or None per slice])
        self.layout_zero = False  # the last op left no layout copy resident
        self.arrays = None        # what resolves a region target (records(spec)); not state

    def __deepcopy__(self, memo):
        new = Model.__new__(Model)
        for k, v in self.__dict__.items():
            new.__dict__[k] = v if k == "arrays" else copy.deepcopy(v, memo)
        return new

    # ---- helpers ----

    def selected(self):
        return self.gmm[self.slot]

    def _drop_query(self, m):
        self.grad[m] = False     # (vr_bake_gradient) the gradient plane goes first
        self.qplane[m] = False

    def _drop_record_planes(self):
        # vr.h (vr_bake_stats): "vr_release_stats drops the copies with the planes"; every
        # query's plane names vr_release_stats, a new upload and vr_convert_f16 among its causes
        for m in QUERIES:
            self._drop_query(m)
        for m in (1, 2, 3):
            self.grad[m] = False
        self.stats = False

    def _drop_codec_planes(self):
        for m in (4, 5, 6):
            self.grad[m] = False
        self.cstats = False

    def plane_resident(self, m):
        if m > G:
            return m - G in self.grad and self.grad[m - G]
        if m in (1, 2, 3):
            return self.stats
        if m in (4, 5, 6):
            return self.cstats
        return self.qplane.get(m, False)

    def query_state(self, m):
        """(set, its bin count or None) of a record query's state"""
        if m == 10:
            return self.weights is not None, self.weights and self.weights["n"]
        if m == 11:
            return self.quant is not None, None
        if m == 12:
            return self.target is not None, self.target and len(self.target["h"])
        return self.xweights is not None, self.xweights and self.xweights["n"]

    def _query_ready(self, m):
        """vr.h (method 10, and alike at 11-13): "VR_ERR_STATE without a record volume,
        without weights, or with a weight count other than the volume's bins;
        VR_ERR_UNSUPPORTED for records of any other bin count" """
        if self.vol is None:
            return ERR_STATE
        if not lin_bins(self.vol["nb"]):
            return ERR_UNSUPPORTED
        is_set, n = self.query_state(m)
        if not is_set or (n is not None and n != self.vol["nb"]):
            return ERR_STATE
        return OK

    def stat_of(self, family, m):
        """the name in random_cases.SPAN of what method m shows now (for draw_window)"""
        if m > G:
            return "grad " + self.stat_of(family, m - G)
        if family == "gmm":
            return {1: "gmm mean", 2: "gmm variance", 10: "range", 13: "crossing",
                    11: "gmm spread" if self.quant and self.quant[2] else "gmm quantile"}.get(
                        m, "range")
        if m == 10:
            return "weights" if self.weights and self.weights["kind"] == "seeded" else "range"
        if m == 11:
            return "spread" if self.quant and self.quant[2] else "quantile"
        return {1: "mean", 2: "variance", 3: "entropy", 7: "mean", 4: "mean", 5: "variance",
                6: "entropy", 12: "distance", 13: "crossing"}[m]

    # ---- ops ----

    def apply(self, op):
        """the status the library must return; on an error "the state stays as it was" """
        self.layout_zero = False
        return getattr(self, "_" + op["op"])(op)

    # volumes

    def _init_distribution(self, op):
        v = op["vol"]
        # vr.h (vr_init_distribution_f16): "nbins must be one of 1, 2, 4, 8, 16, 32
        # (VR_ERR_UNSUPPORTED otherwise)"
        if v["dtype"] == "f16" and not lin_bins(v["nb"]):
            return ERR_UNSUPPORTED
        self._drop_record_planes()
        self.vol = dict(v, narrowed=False)
        self.layout_zero = True
        return OK

    def _convert_f16(self, op):
        # vr.h (vr_convert_f16): "VR_ERR_STATE if no volume is resident or it is f16 already"
        if self.vol is None or self.vol["dtype"] == "f16" or self.vol["narrowed"]:
            return ERR_STATE
        if not lin_bins(self.vol["nb"]):
            return ERR_UNSUPPORTED
        self._drop_record_planes()
        self.vol = dict(self.vol, narrowed=True, adopt=False)   # "a new library-owned buffer"
        self.layout_zero = True
        return OK

    def _init_codec(self, op):
        self._drop_codec_planes()
        self.codec = dict(op["codec"])
        return OK

    def _freeCudaBuffers(self, op):
        # vr.h (vr_gmm_select): "vr_free_gmm frees only it, freeCudaBuffers both"
        self._drop_record_planes()
        self._drop_codec_planes()
        self.vol = self.codec = None
        self.gmm, self.slot = [None, None], 0
        self.gplanes = {k: None for k in GMM_SETS}
        self.layout_zero = True
        return OK

    def _init_gmm(self, op):
        g, zb, ns = op["gmm"], op["z_base"], op["nslices"]
        if g["K"] not in (8, 16, 32):
            return ERR_UNSUPPORTED
        if zb < 0 or ns < 1 or zb + ns > g["dims"][2]:
            return ERR_ARG
        # vr.h (vr_init_gmm): "A new GMM volume replaces the previous one"; (vr_bake_gmm_stats)
        # "The planes belong to no slot and to no resident records: they survive vr_init_gmm*"
        self.gmm[self.slot] = dict(spec=dict(g, narrowed=False), z_base=zb, nzs=ns)
        return OK

    def _free_gmm(self, op):
        self.gmm[self.slot] = None
        return OK

    def _gmm_select(self, op):
        if op["slot"] not in (0, 1):
            return ERR_ARG
        self.slot = op["slot"]
        return OK

    def _convert_gmm_f16(self, op):
        # vr.h (vr_convert_gmm_f16): "VR_ERR_STATE if the slot holds no volume or it is f16 already"
        v = self.selected()
        if v is None or v["spec"]["dtype"] == "f16" or v["spec"]["narrowed"]:
            return ERR_STATE
        v["spec"] = dict(v["spec"], narrowed=True)
        return OK

    # bakes and releases

    def _bake_stats(self, op):
        if self.vol is None and self.codec is None:
            return ERR_STATE
        # vr.h (vr_bake_stats): "bakes the planes of the resident raw and codec volumes that
        # are not baked yet"
        self.stats = self.stats or self.vol is not None
        self.cstats = self.cstats or self.codec is not None
        return OK

    def _release_stats(self, op):
        self._drop_record_planes()
        self._drop_codec_planes()
        self.layout_zero = True
        return OK

    def _bake_query(self, m):
        rc_ = self._query_ready(m)
        if rc_ != OK:
            return rc_
        self.qplane[m] = True
        return OK

    def _release_query(self, m):
        self._drop_query(m)
        return OK

    def _bake_weighted(self, op): return self._bake_query(10)
    def _bake_quantile(self, op): return self._bake_query(11)
    def _bake_distance(self, op): return self._bake_query(12)
    def _bake_crossing(self, op): return self._bake_query(13)
    def _release_weighted(self, op): return self._release_query(10)
    def _release_quantile(self, op): return self._release_query(11)
    def _release_distance(self, op): return self._release_query(12)
    def _release_crossing(self, op): return self._release_query(13)

    def _bake_gradient(self, op):
        # vr.h (vr_bake_gradient): "VR_ERR_ARG for an m that is no source, VR_ERR_STATE if
        # m's plane is not resident (bake it first); nothing to do if the gradient plane is there"
        m = op["m"]
        if m not in SOURCES:
            return ERR_ARG
        if not self.plane_resident(m):
            return ERR_STATE
        self.grad[m] = True
        return OK

    def _release_gradient(self, op):
        if op["m"] not in SOURCES:
            return ERR_ARG
        self.grad[op["m"]] = False
        return OK

    def _bake_gmm(self, name, ready):
        # vr.h (vr_bake_gmm_stats): "VR_ERR_STATE: no GMM volume in the selected slot";
        # "later calls must come from a volume of the same dims (VR_ERR_STATE otherwise)";
        # (vr_bake_gmm_range) "VR_ERR_STATE: no GMM volume in the selected slot, no range
        # set, or other dims"
        v = self.selected()
        if v is None or not ready:
            return ERR_STATE
        p = self.gplanes[name]
        dims = tuple(v["spec"]["dims"])
        if p is not None and tuple(p["dims"]) != dims:
            return ERR_STATE
        if p is None:
            p = self.gplanes[name] = dict(dims=dims, src=[None] * dims[2])
        for z in range(v["z_base"], v["z_base"] + v["nzs"]):
            p["src"][z] = dict(v["spec"])   # "Baking a slice again is allowed"
        return OK

    def _bake_gmm_stats(self, op): return self._bake_gmm("stats", True)
    def _bake_gmm_range(self, op): return self._bake_gmm("range", self.gmm_range is not None)
    def _bake_gmm_quantile(self, op): return self._bake_gmm("quant", self.quant is not None)

    def _release_gmm(self, name):
        self.gplanes[name] = None
        return OK

    def _release_gmm_stats(self, op): return self._release_gmm("stats")
    def _release_gmm_range(self, op): return self._release_gmm("range")
    def _release_gmm_quantile(self, op): return self._release_gmm("quant")

    # the caller's state

    def _set_bin_weights(self, op):
        # vr.h (vr_set_bin_weights): "n in 1, 2, 4, 8, 16, 32, else VR_ERR_UNSUPPORTED; every
        # weight finite, else VR_ERR_ARG"; "Setting or clearing weights drops the baked
        # weighted plane"
        w = op["w"]
        if not lin_bins(w["n"]):
            return ERR_UNSUPPORTED
        if op.get("poison"):
            return ERR_ARG
        self._drop_query(10)
        self.weights = dict(w)
        return OK

    def _clear_bin_weights(self, op):
        self._drop_query(10)
        self.weights = None
        return OK

    def _set_query_range(self, op):
        # vr.h (vr_set_query_range): "lo > hi or a non-finite bound: VR_ERR_ARG; n as for
        # vr_set_bin_weights"
        lo, hi, n = op["lo"], op["hi"], op["n"]
        if not lin_bins(n):
            return ERR_UNSUPPORTED
        if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
            return ERR_ARG
        self._drop_query(10)
        self.weights = dict(kind="range", lo=lo, hi=hi, n=n)
        return OK

    def _quantile_set(self, lo, hi, spread):
        # vr.h (vr_set_quantile): "q finite and in [0, 1], q_lo <= q_hi, else VR_ERR_ARG and
        # the state stays as it was"; "Each of the three drops the baked quantile plane, and
        # the quantile plane of GMM volumes"
        if not all(math.isfinite(q) and 0.0 <= q <= 1.0 for q in (lo, hi)) or lo > hi:
            return ERR_ARG
        self._drop_query(11)
        self.gplanes["quant"] = None
        self.quant = (_f32(lo), _f32(hi), spread)
        return OK

    def _set_quantile(self, op): return self._quantile_set(op["q"], op["q"], False)
    def _set_quantile_spread(self, op): return self._quantile_set(op["lo"], op["hi"], True)

    def _clear_quantile(self, op):
        self._drop_query(11)
        self.gplanes["quant"] = None
        self.quant = None
        return OK

    def _set_query_target(self, op):
        # vr.h (vr_set_query_target): "n in 1, 2, 4, 8, 16, 32, else VR_ERR_UNSUPPORTED; every
        # h_i finite and metric in 0 .. 2, else VR_ERR_ARG; an error leaves the state as it was"
        if not lin_bins(len(op["h"])):
            return ERR_UNSUPPORTED
        if op["metric"] not in rc.METRICS or not all(math.isfinite(v) for v in op["h"]):
            return ERR_ARG
        self._drop_query(12)   # "Every call that sets or clears the target drops the baked distance plane"
        self.target = dict(h=[_f32(v) for v in op["h"]], metric=op["metric"],
                           similarity=bool(op["similarity"]))
        return OK

    def _clear_query_target(self, op):
        self._drop_query(12)
        self.target = None
        return OK

    def _set_query_target_region(self, op):
        # vr.h (vr_set_query_target_region): "The box must be non-empty, inside the volume
        # and of at most 4096 voxels, else VR_ERR_ARG; VR_ERR_STATE without a record volume"
        if self.vol is None:
            return ERR_STATE
        lo, hi = op["lo"], op["hi"]
        if any(a < 0 or b > n or a >= b for a, b, n in zip(lo, hi, self.vol["dims"])) or \
                int(np.prod([b - a for a, b in zip(lo, hi)])) > 4096:
            return ERR_ARG
        if not lin_bins(self.vol["nb"]):
            return ERR_UNSUPPORTED
        if op["metric"] not in rc.METRICS:
            return ERR_ARG
        # "The state is then that of vr_set_query_target, and vr_query_target reads it back"
        if self.arrays is None:   # (the generator: the values matter to no decision)
            h = [0.0] * self.vol["nb"]
        else:
            import ref_distance
            h = [float(v) for v in ref_distance.region_mean(self.arrays.records(self.vol), lo, hi)]
        self._drop_query(12)
        self.target = dict(h=h, metric=op["metric"], similarity=bool(op["similarity"]))
        return OK

    def _set_isovalue(self, op):
        # vr.h (vr_set_isovalue): "bit for bit the weights vr_set_query_range(0, theta, n)
        # makes"; "theta must be finite, else VR_ERR_ARG"
        if not lin_bins(op["n"]):
            return ERR_UNSUPPORTED
        if not math.isfinite(op["theta"]):
            return ERR_ARG
        self._drop_query(13)   # "Every call that sets or clears the crossing weights drops the crossing plane"
        self.xweights = dict(kind="isovalue", lo=0.0, hi=op["theta"], n=op["n"])
        return OK

    def _set_crossing_weights(self, op):
        w = op["w"]
        if not lin_bins(w["n"]):
            return ERR_UNSUPPORTED
        if op.get("poison"):
            return ERR_ARG
        self._drop_query(13)
        self.xweights = dict(w)
        return OK

    def _clear_crossing_weights(self, op):
        self._drop_query(13)
        self.xweights = None
        return OK

    def _set_gmm_range(self, op):
        # vr.h (vr_set_gmm_range): "NaN or lo > hi: VR_ERR_ARG, the state stays as it was;
        # +-inf is allowed"; "Both drop the baked range plane"
        lo, hi = op["lo"], op["hi"]
        if math.isnan(lo) or math.isnan(hi) or lo > hi:
            return ERR_ARG
        self.gplanes["range"] = None
        self.gmm_range = (_f32(lo), _f32(hi))
        return OK

    def _clear_gmm_range(self, op):
        self.gplanes["range"] = None
        self.gmm_range = None
        return OK

    def _set_transfer_function(self, op):
        # vr.h (vr_set_transfer_function): "n outside 1 .. VR_TF_MAX or a value that is not
        # finite: VR_ERR_ARG, the state stays as it was"; "a successful
        # vr_set_transfer_function(non-NULL) clears the 2-D table; a NULL call clears only
        # this one"; "It drops no baked plane"
        t = op["table"]
        if t is None:
            self.tf = None
            return OK
        if not 1 <= t["shape"][0] <= 256 or op.get("poison"):
            return ERR_ARG
        self.tf, self.tf2 = dict(t), None
        return OK

    def _set_transfer_function_2d(self, op):
        # vr.h (vr_set_transfer_function_2d): "nu or nv outside 1 .. 256, nu * nv >
        # VR_TF2_MAX, a table value, v_offset or v_scale that is not finite, or a method_v
        # outside {1, 2, 3, 4, 5, 6, 10, 11, 12, 13}: VR_ERR_ARG"; gradient methods are v
        # planes too (vr_bake_gradient: "as u or as method_v of the 2-D table")
        t = op["table"]
        if t is None:
            self.tf2 = None
            return OK
        nv, nu = t["shape"]
        mv = op["mv"]
        if not (1 <= nu <= 256 and 1 <= nv <= 256 and nu * nv <= 1024) or op.get("poison"):
            return ERR_ARG
        if mv not in SOURCES and mv - G not in SOURCES:
            return ERR_ARG
        if not (math.isfinite(op["voff"]) and math.isfinite(op["vscale"])):
            return ERR_ARG
        self.tf2 = dict(table=dict(t), mv=mv, voff=_f32(op["voff"]), vscale=_f32(op["vscale"]))
        self.tf = None
        return OK

    def _set_projection(self, op):
        # vr.h (vr_set_projection): "one of the four modes; anything else is VR_ERR_ARG and
        # the state stays as it was"
        if op["mode"] is not None and op["mode"] not in PROJECTIONS:
            return ERR_ARG
        self.proj = op["mode"]
        return OK

    def _set_light(self, op):
        # vr.h (vr_set_light): "A coefficient that is not finite or is negative, or
        # shininess_log2 outside 0..7, is VR_ERR_ARG and the state stays as it was"
        lt = op["light"]
        if lt is None:
            self.light = None
            return OK
        if not all(math.isfinite(c) and c >= 0 for c in lt[:3]) or not 0 <= lt[3] <= 7:
            return ERR_ARG
        self.light = tuple(_f32(c) for c in lt[:3]) + (int(lt[3]),)
        return OK

    def _set_stream(self, op):
        self.stream = op["which"]
        return OK

    def _set_layout_budget(self, op):
        # vr.h (vr_set_layout_budget): "drops resident copies that exceed a lowered budget"
        self.budget = op["bytes"]
        self.layout_zero = op["bytes"] == 0
        return OK

    def _set_tuning(self, op):
        if op["value"] is None:
            self.knobs.pop(op["key"], None)
        else:
            self.knobs[op["key"]] = op["value"]
        return OK

    # ---- what the getters must report ----

    def census(self):
        v, gv = self.vol, self.selected()
        sets = {}
        for name, p in self.gplanes.items():
            sets[name] = (p is not None, 0 if p is None else sum(s is not None for s in p["src"]))
        tf2 = None
        if self.tf2 is not None:
            tf2 = (table_value(self.tf2["table"]), self.tf2["mv"], self.tf2["voff"], self.tf2["vscale"])
        t = self.target
        return {
            "weighted_info": self.qplane[10], "quantile_info": self.qplane[11],
            "distance_info": self.qplane[12], "crossing_info": self.qplane[13],
            "gradient_info": {m: self.grad[m] for m in SOURCES},
            "stats_info": (self.stats, self.cstats),
            "gmm_stats_info": sets["stats"], "gmm_range_info": sets["range"],
            "gmm_quantile_info": sets["quant"],
            "bin_weights": weights_value(self.weights), "quantile": self.quant,
            "query_target": None if t is None else (np.array(t["h"], np.float32), t["metric"],
                                                    t["similarity"]),
            "crossing_weights": weights_value(self.xweights), "gmm_range": self.gmm_range,
            "transfer_function": None if self.tf is None else table_value(self.tf),
            "transfer_function_2d": tf2, "projection": self.proj,
            "light": None if self.light is None else dict(
                ambient=self.light[0], diffuse=self.light[1], specular=self.light[2],
                shininess=1 << self.light[3]),
            "volume_dtype": None if v is None else
            ("f16" if v["dtype"] == "f16" or v["narrowed"] else "f32"),
            "gmm_dtype": None if gv is None else
            ("f16" if gv["spec"]["dtype"] == "f16" or gv["spec"]["narrowed"] else "f32"),
            # vr.h (vr_bake_stats, vr_convert_f16, vr_set_layout_budget): no copy outlives the
            # records it was made from, the planes' release or a budget of 0
            "layout_zero": self.layout_zero,
        }

    # ---- what a frame must be ----

    def expect(self, probe):
        """{"status", "why"} of the refusal (vr.h, vr_set_transfer_function: "The order of the
        checks, where more than one refusal applies to a frame"), or the recipe of the frame:
        {"family", "route", "u", "v", "bar"} -- march the records or the planes of the
        current state by `route` (march: per step; plane: the baked plane under the built-in
        table; tf, tf2, proj, lit) and compare at `bar` (same: bit for bit; parity:
        test_gpu_parity.assert_parity; gmm: test_gpu_gmm.check).  render_frame's precedence:
        light, then projection, then the 1-D table, then the 2-D table, then the plain march."""
        entry, m = probe["entry"], probe["method"]
        why = []   # (status, reason) in the library's order of checks
        if entry == "render":
            recipe = self._expect_render(m, why)
        elif entry == "render_gmm":
            recipe = self._expect_render_gmm(m, why)
        else:
            recipe = self._expect_render_gmm_baked(m, why)
        if why:
            return dict(status=why[0][0], why=why[0][1], several=len({s for s, _ in why}) > 1)
        return recipe

    def _route(self):
        return "lit" if self.light else "proj" if self.proj else "tf" if self.tf else \
            "tf2" if self.tf2 else None

    def _conflicts(self, why):
        # vr.h (vr_set_projection): "any frame while a 2-D table is set (a projection
        # classifies one plane) -- is VR_ERR_UNSUPPORTED"; (vr_set_light) "any frame while a
        # 2-D table is set and any frame while a projection is set ... is VR_ERR_UNSUPPORTED"
        if self.light and self.proj:
            why.append((ERR_UNSUPPORTED, "light over projection"))
        if self.light and self.tf2:
            why.append((ERR_UNSUPPORTED, "light over 2-D table"))
        if self.proj and self.tf2 and not self.light:
            why.append((ERR_UNSUPPORTED, "projection over 2-D table"))

    def _expect_render(self, m, why):
        src = m - G if m > G else 0
        valid = m in (1, 2, 3, 4, 5, 6, 7) or m in QUERIES or src in SOURCES
        if not valid:
            why.append((ERR_ARG, "unknown method"))
            return None
        # vr.h (vr_bake_gradient): "with its plane not resident every frame of it is
        # VR_ERR_UNSUPPORTED (vr_bake_gradient first)"
        if src and not self.grad[src]:
            why.append((ERR_UNSUPPORTED, "gradient plane not baked"))
        family = plane_family(m) or "records"
        if family == "codec" and self.codec is None:
            why.append((ERR_STATE, "no codec volume"))
        if family == "records" and self.vol is None:
            why.append((ERR_STATE, "no record volume"))
        if m in QUERIES and self.vol is not None:
            st = self._query_ready(m)
            if st != OK:
                why.append((st, "query state"))
        route = self._route()
        self._conflicts(why)
        v = None
        if route in ("lit", "proj", "tf"):
            # vr.h (vr_set_transfer_function): "While a table is set a frame comes from a
            # baked plane or not at all"; the projection and the light "serve exactly the
            # frames a 1-D table serves"
            if not self.plane_resident(m):
                why.append((ERR_UNSUPPORTED, f"{route}: no baked plane"))
        elif route == "tf2":
            # vr.h (vr_set_transfer_function_2d): "a plane that is not resident, or a u /
            # method_v pair of different families: VR_ERR_UNSUPPORTED"
            v = self.tf2["mv"]
            if plane_family(m) is None or plane_family(m) != plane_family(v) or \
                    not self.plane_resident(m) or not self.plane_resident(v):
                why.append((ERR_UNSUPPORTED, "tf2: planes"))
        elif m == 7 and self.vol is not None and not self.stats and \
                (self.vol["dtype"] == "f16" or self.vol["narrowed"]):
            # vr.h (vr_init_distribution_f16): "Method 7 on an unbaked f16 volume is
            # VR_ERR_UNSUPPORTED (bake first)"
            why.append((ERR_UNSUPPORTED, "method 7 on unbaked f16 records"))
        if route is None:
            route = "plane" if (src or (m in QUERIES and self.qplane[m])) else "march"
        bar = "parity" if route == "march" and m in (1, 2, 3, 4, 5, 6, 7) else "same"
        return dict(family=family, route=route, u=m, v=v, bar=bar)

    def _expect_render_gmm(self, m, why):
        # vr.h (vr_set_transfer_function, vr_set_projection, vr_set_light): vr_render_gmm is
        # among "everything else"
        if self.light or self.proj or self.tf or self.tf2:
            why.append((ERR_UNSUPPORTED, "vr_render_gmm under a table, projection or light"))
        gv = self.selected()
        if gv is None:
            why.append((ERR_STATE, "no GMM volume"))
        # vr.h (vr_init_gmm_f16): "queryMethod 1 and 2, 10 once a range is set ... and 11 once
        # a quantile is set ..., anything else VR_ERR_UNSUPPORTED"
        if m not in (1, 2, 10, 11):
            why.append((ERR_UNSUPPORTED, "method"))
        if (m == 10 and self.gmm_range is None) or (m == 11 and self.quant is None):
            why.append((ERR_STATE, "query state"))
        # vr.h (vr_render_gmm): "slab == NULL renders the whole frame (all slices must be
        # resident)"
        if gv is not None and (gv["z_base"] != 0 or gv["nzs"] != gv["spec"]["dims"][2]):
            why.append((ERR_STATE, "slices missing"))
        return dict(family="gmm", route="march", u=m, v=None, bar="gmm" if m <= 2 else "same")

    def _gmm_set(self, m):
        return next((k for k, ms in GMM_SETS.items() if m in ms), None)

    def _expect_render_gmm_baked(self, m, why):
        # vr.h (vr_render_gmm_baked): "a whole frame of queryMethod 1 or 2 (10 ...; 11 ...;
        # others: VR_ERR_UNSUPPORTED) from the planes; VR_ERR_STATE unless all Z slices are
        # baked"; (vr_bake_gradient) "vr_render_gmm_baked with a gradient method ... is
        # VR_ERR_UNSUPPORTED"
        name = self._gmm_set(m)
        if name is None:
            why.append((ERR_UNSUPPORTED, "method"))
            return None
        p = self.gplanes[name]
        route = self._route()
        self._conflicts(why)
        complete = p is not None and all(s is not None for s in p["src"])
        if p is None:
            # vr.h (the order of the checks): the light and the 2-D table name the missing
            # plane set as their refusal; "as without any of them and so under a 1-D table or
            # a projection too, VR_ERR_STATE for a plane set that is not baked or not complete"
            if route in ("lit", "tf2"):
                why.append((ERR_UNSUPPORTED, f"{route}: no baked plane"))
            else:
                why.append((ERR_STATE, "no baked GMM planes"))
        elif not complete:
            why.append((ERR_STATE, "slices missing"))
        v = None
        if route == "tf2":
            # vr.h (vr_set_transfer_function_2d): "every plane set used complete (else
            # VR_ERR_STATE, as without a table) and of the same dimensions (else VR_ERR_STATE)"
            v = self.tf2["mv"]
            vname = self._gmm_set(v)
            q = self.gplanes[vname] if vname else None
            if q is None:
                why.append((ERR_UNSUPPORTED, "tf2: v plane"))
            elif not all(s is not None for s in q["src"]):
                why.append((ERR_STATE, "tf2: v slices missing"))
            elif p is not None and tuple(q["dims"]) != tuple(p["dims"]):
                why.append((ERR_STATE, "tf2: dims differ"))
        return dict(family="gmm", route=route or "plane", u=m, v=v, bar="same")


# ---------------------------------------------------------------- the generator

# the caller's state, one change inside every scene (after its planes are resident, before
# the cause of their drop), in turn: every pair of light, projection and 2-D table stands
# against each other once per turn.  The volume scenes clear all of it instead, so that a
# per-step frame can show the new contents.
SPRINKLES = ("proj on", "tf2 on", "all off", "tf2 on", "light on", "all off", "light on",
             "proj on", "all off", "tf on", "light on", "all off")
# and after the scenes: the stream scene where it fits (_Gen.stream_scene), then the layout
# budget and a knob
SPRINKLES_B = ("budget 0", "knob", "budget default", "knob off")
BAD = ("quantile", "range nan", "table 257", "bake without state", "spread order", "weights 3",
       "gmm range order", "light negative", "projection 4", "tf2 method 7", "isovalue nan",
       "gradient 7", "gradient without source", "metric 5", "slot 2", "convert twice",
       "region outside", "gmm range nan", "bake gmm without state", "table nan", "weights inf",
       "tf2 too large")

# A scene makes planes resident and applies one documented cause of their drop.
#   own:    a record query's plane, dropped by one of its own calls; event i: family i % 4,
#           and (i // 4) % 3: the first setter, the release and after a rebake the clear,
#           the second setter
#   volume: the statistics planes and two queries' planes, dropped by what replaces or
#           releases the records; scene i: cause i % 7, queries (i // 7) % 2
#   codec:  the codec planes; scene i: cause i % 3
#   gmm:    GMM_SCENES in turn
OWN_CAUSES = {10: ("set_bin_weights", "release_weighted", "set_query_range", "clear_bin_weights"),
              11: ("set_quantile", "release_quantile", "set_quantile_spread", "clear_quantile"),
              12: ("set_query_target", "release_distance", "set_query_target_region",
                   "clear_query_target"),
              13: ("set_isovalue", "release_crossing", "set_crossing_weights",
                   "clear_crossing_weights")}
VOLUME_CAUSES = ("upload", "convert_f16", "release_stats", "upload", "convert_f16",
                 "freeCudaBuffers", "upload")
CODEC_CAUSES = ("init_codec", "release_stats", "freeCudaBuffers")
GMM_SCENES = (("gmm", "stats", "release_gmm_stats"), ("gmm", "range", "set_gmm_range"),
              ("gmm", "quant", "set_quantile"), ("gmm survive", "init_gmm", None),
              ("gmm", "range", "clear_gmm_range"), ("gmm", "quant", "set_quantile_spread"),
              ("gmm slabs", "stats", None), ("gmm", "stats", "freeCudaBuffers"),
              ("gmm", "range", "release_gmm_range"), ("gmm", "quant", "clear_quantile"),
              ("gmm survive", "free_gmm", None), ("gmm", "range", "freeCudaBuffers"),
              ("gmm", "quant", "release_gmm_quantile"), ("gmm survive", "gmm_select", None),
              ("gmm slabs", "range", None), ("gmm", "quant", "freeCudaBuffers"),
              ("gmm survive", "convert_gmm_f16", None), ("gmm slabs", "quant", None))


class _Full(Exception):
    """a session holds at most 20 ops"""


class _Gen:
    def __init__(self, seed):
        self.seed, self.flavour, self.turn = seed, FLAVOURS[seed % 4], seed // 4
        self.rng = np.random.default_rng(13000 + seed)
        self.model = Model()
        self.ops = []
        self.next_seed = 1000 * seed
        self.nbad = 0
        self.last_nb = 0
        self.stat_due = 0
        self.no_bad = False
        # every second records session starts with the layout scene
        self.layout = self.flavour == "records" and self.turn % 2 == 0
        self.sprinkle_at = (5 * seed + seed // 12) % len(SPRINKLES)
        self.sprinkle_b = (seed + seed // 4) % len(SPRINKLES_B)

    # ---- emitting ----

    def emit(self, **op):
        if len(self.ops) >= 20:
            raise _Full
        m = self.model
        probe = op.pop("force_probe", None)
        op["status"] = m.apply(op)
        op["probe"] = probe or self.deal_probe(op)
        op["refuse"] = self.deal_refusal()
        # one step in four, or the next one after it at which a plane is resident
        self.stat_due += 1
        op["stat"] = self.deal_stat() if self.stat_due >= 4 else None
        if op["stat"] is not None:
            self.stat_due = 0
        self.ops.append(op)
        # one op in about ten is a bad call
        if op["status"] == OK and not self.no_bad and (len(self.ops) + self.seed) % 11 == 4:
            self.bad_call()

    def fresh_seed(self):
        self.next_seed += 1
        return self.next_seed

    # ---- volumes ----

    def new_vol(self, like=None, dtype=None):
        rng = self.rng
        if like is not None:
            dims, nb = tuple(like["dims"]), like["nb"]
        else:
            dims = tuple(int(v) for v in rng.integers(2, 25, 3))
            if rng.integers(0, 4) == 0:   # around the planes' 15-voxel pitch, odd row counts
                dims = (int(rng.choice(rc.EDGE_NX)), int(rng.choice(rc.EDGE_NY)), dims[2])
            nb = int(rng.choice(rc.INSTANCE_BINS))
            if self.last_nb and rng.integers(0, 4):   # mostly the bins the caller's state is for
                nb = self.last_nb
        self.last_nb = nb
        dtype = dtype or ("f32", "f32", "f16")[int(rng.integers(0, 3))]
        return dict(dims=dims, nb=nb, dtype=dtype, seed=self.fresh_seed(),
                    adopt=bool(rng.integers(0, 5) == 0))

    def new_gmm(self, like=None, dtype=None):
        rng = self.rng
        if like is not None:
            dims, K = tuple(like["dims"]), like["K"]
        else:
            dims = tuple(int(v) for v in rng.integers(2, 17, 3))
            K = int(rng.choice([8, 16, 32]))
        dtype = dtype or ("f32", "f16")[int(rng.integers(0, 2))]
        return dict(dims=dims, K=K, dtype=dtype, seed=self.fresh_seed())

    def first(self):
        """the first volumes and a state for their queries"""
        self.no_bad = True
        if self.flavour != "gmm":
            vol = self.new_vol()
            if self.layout:   # what gets an axis-rows copy at this size: owned fp32 records of
                # 1, 2 or 4 bins (8-bin records of a volume this coarse for its frame take the
                # LDS-box march on the x rows instead: vr_plan.cpp)
                vol.update(dtype="f32", adopt=False, nb=min(vol["nb"], 4))
                self.last_nb = vol["nb"]
            self.emit(op="init_distribution", vol=vol)
            for m in QUERIES:
                self.set_state(m)
        if self.flavour == "records+codec":
            self.ensure_codec()
        if self.flavour in ("gmm", "mixed"):
            self.ensure_gmm()
            self.set_gmm_state("range")
            if self.model.quant is None:
                self.set_gmm_state("quant")
        first, self.ops, self.no_bad = self.ops, [], False
        return first

    def ensure_records(self, dtype=None):
        v = self.model.vol
        if v is None:
            self.emit(op="init_distribution", vol=self.new_vol(dtype=dtype))
        elif dtype == "f32" and (v["dtype"] == "f16" or v["narrowed"]):
            self.emit(op="init_distribution", vol=self.new_vol(like=v, dtype="f32"))

    def ensure_codec(self):
        if self.model.codec is None:
            rng = self.rng
            dims = tuple(int(v) for v in rng.integers(2, 25, 3))
            self.emit(op="init_codec", codec=dict(dims=dims, nb=int(rng.choice(rc.INSTANCE_BINS)),
                                                  seed=self.fresh_seed()))

    def ensure_gmm(self, dtype=None, whole=True):
        v = self.model.selected()
        spec = v and v["spec"]
        if v is None or (whole and v["nzs"] != spec["dims"][2]) or \
                (dtype == "f32" and (spec["dtype"] == "f16" or spec["narrowed"])):
            g = self.new_gmm(dtype=dtype)
            self.emit(op="init_gmm", gmm=g, z_base=0, nslices=g["dims"][2])

    # ---- the caller's state ----

    def set_state(self, m, how=None):
        """a new state of record query m, by the setter `how` (None: either)"""
        rng, nb = self.rng, self.model.vol["nb"] if self.model.vol else 8
        if m == 10:
            how = how or ("set_bin_weights", "set_query_range")[int(rng.integers(0, 2))]
            if how == "set_bin_weights":
                self.emit(op=how, w=dict(kind="seeded", wseed=int(rng.integers(1, 1 << 20)), n=nb))
            else:
                lo, hi = rc._ordered_pair(rng)
                self.emit(op=how, lo=lo, hi=hi, n=nb)
        elif m == 11:
            how = how or ("set_quantile", "set_quantile_spread")[int(rng.integers(0, 3) == 0)]
            if how == "set_quantile":
                self.emit(op=how, q=_f32(rng.uniform(0.02, 0.98)))
            else:
                lo, hi = rc._ordered_pair(rng)
                self.emit(op=how, lo=lo, hi=hi)
        elif m == 12:
            how = how or ("set_query_target", "set_query_target_region")[int(rng.integers(0, 2))]
            metric, sim = rc.METRICS[int(rng.integers(0, 3))], bool(rng.integers(0, 2))
            if how == "set_query_target" or self.model.vol is None:
                h = rng.random(nb) + 0.05
                self.emit(op="set_query_target", h=[_f32(v) for v in h / h.sum()], metric=metric,
                          similarity=sim)
            else:
                lo, hi = [], []
                for n in self.model.vol["dims"]:
                    a = int(rng.integers(0, n))
                    lo.append(a)
                    hi.append(int(rng.integers(a + 1, min(n, a + 4) + 1)))
                self.emit(op=how, lo=tuple(lo), hi=tuple(hi), metric=metric, similarity=sim)
        else:
            how = how or ("set_isovalue", "set_crossing_weights")[int(rng.integers(0, 3) == 0)]
            if how == "set_isovalue":
                self.emit(op=how, theta=_f32(rng.uniform(0.05, 0.95)), n=nb)
            else:   # F = P(lo <= v < hi): any probability linear in the bins may stand for F
                lo, hi = rc._ordered_pair(rng)
                self.emit(op=how, w=dict(kind="range", lo=lo, hi=hi, n=nb))

    def ensure_state(self, m):
        is_set, n = self.model.query_state(m)
        if not is_set or (n is not None and n != self.model.vol["nb"]):
            self.set_state(m)

    def ensure_plane(self, m):
        """the plane of source method m resident (records or codec)"""
        if m in (4, 5, 6):
            self.ensure_codec()
            if not self.model.cstats:
                self.emit(op="bake_stats")
            return
        self.ensure_records()
        if m in (1, 2, 3):
            if not self.model.stats:
                self.emit(op="bake_stats")
            return
        self.ensure_state(m)
        if not self.model.qplane[m]:
            self.emit(op="bake_" + QUERY_NAME[m])

    def set_gmm_state(self, name, how=None):
        rng = self.rng
        if name == "range":
            lo, hi = rc._ordered_pair(rng)
            k = int(rng.integers(0, 4))
            lo, hi = (-math.inf, hi) if k == 0 else (lo, math.inf) if k == 1 else (lo, hi)
            self.emit(op="set_gmm_range", lo=lo, hi=hi)
        elif name == "quant":
            self.set_state(11, how)

    def ensure_gmm_plane(self, name):
        m = self.model
        self.ensure_gmm()
        if name == "range" and m.gmm_range is None:
            self.set_gmm_state("range")
        if name == "quant" and m.quant is None:
            self.set_gmm_state("quant")
        p, spec = m.gplanes[name], m.selected()["spec"]
        # vr.h (vr_bake_gmm_stats): "A CALLER WHO CHANGES THE VOLUME'S RECORDS ... MUST CALL
        # vr_release_gmm_stats BEFORE BAKING AGAIN"; other dims need it too
        if p is not None and (tuple(p["dims"]) != tuple(spec["dims"]) or
                              any(s is not None and s != spec for s in p["src"])):
            self.emit(op="release_gmm_" + GMM_NAME[name])
        p = m.gplanes[name]
        if p is None or any(s is None for s in p["src"]):
            self.emit(op="bake_gmm_" + GMM_NAME[name])

    # ---- scenes ----

    def layout_scene(self):
        """The knob with which tests/test_gpu_layout.py makes the plan take layout copies at
        small sizes, then a side view of the records per step: an axis-rows copy of the
        owned fp32 volume (vr.h, vr_bake_stats: "Views whose screen x runs along the volume's
        z or y axis ... of an owned volume with 1, 2, 4 or 8 bins get an axis-rows copy"),
        resident until a later op of the session replaces or releases the records."""
        rot = ((0.0, 90.0), (90.0, 90.0))[self.turn // 2 % 2]
        probe = dict(entry="render", method=(1, 2, 3)[self.turn // 2 % 3], W=64, H=48, kind=1,
                     rotation=rot, translation=(0.0, 0.0, -4.0),
                     params=dict(density=0.05, brightness=1.0, toff=0.0, tscale=1.0))
        self.emit(op="set_tuning", key="VR_SEG_RAYS", value="0", force_probe=probe)

    def reshape_scene(self):
        """new records of other dims over resident planes: nothing of the old shape may
        serve a frame of the new one"""
        self.ensure_plane(1)
        v = self.model.vol
        new = self.new_vol(like=v)
        while tuple(new["dims"]) == tuple(v["dims"]):
            new["dims"] = tuple(int(n) for n in self.rng.integers(2, 25, 3))
        if self.turn % 4 == 1:   # and of other bins
            new["nb"] = int([b for b in rc.INSTANCE_BINS if b != v["nb"]][self.turn % 5])
            self.last_nb = new["nb"]
        self.emit(op="init_distribution", vol=new)

    def gradient(self, m, how):
        """how 1: the gradient plane of m resident (it goes with its source); 2: baked and
        released again"""
        if how:
            self.emit(op="bake_gradient", m=m)
        if how == 2:
            self.emit(op="release_gradient", m=m)

    def scene(self, scene, i):
        kind, a, b = scene
        if kind == "own":
            m, how = (10, 11, 12, 13)[i % 4], (i // 4) % 3
            setter1, release, setter2, clear = OWN_CAUSES[m]
            self.ensure_plane(m)
            if how != 1:   # of a family's eight such events three keep the gradient plane
                j = i // 4 - i // 12   # for the cause, three release it first, two bake none
                self.gradient(m, (1, 2, 1 if j < 4 else 2, 0)[j % 4])
            self.sprinkle()
            if how == 1:   # the release, and after a rebake the clear
                self.emit(op=release)
                self.ensure_plane(m)
                self.emit(op=clear)
            else:
                self.set_state(m, setter2 if how else setter1)
        elif kind == "volume":
            cause, pair = VOLUME_CAUSES[i % 7], ((10, 11), (12, 13))[(i // 7) % 2]
            self.ensure_records(dtype="f32" if cause == "convert_f16" else None)
            self.ensure_plane(1)
            for m in pair:
                self.ensure_plane(m)
            self.gradient((1, 2, 3)[i % 3], 2 if i % 4 == 3 else 1)
            self.all_off()
            if cause == "upload":   # new contents of the same dims and bins
                self.emit(op="init_distribution", vol=self.new_vol(like=self.model.vol))
            else:
                self.emit(op=cause)
        elif kind == "codec":
            cause = CODEC_CAUSES[i % 3]
            self.ensure_plane(4)
            self.gradient(4 + (i // 3 + i) % 3, 1 + (i // 3) % 2)
            if cause == "init_codec":
                self.emit(op="init_codec", codec=dict(self.model.codec, seed=self.fresh_seed()))
            else:
                self.emit(op=cause)
        elif kind == "gmm":
            self.ensure_gmm_plane(a)
            self.sprinkle()
            if b == "set_gmm_range":
                self.set_gmm_state("range")
            elif b in ("set_quantile", "set_quantile_spread"):
                self.set_gmm_state("quant", b)
            else:
                self.emit(op=b)
        elif kind == "gmm survive":
            name = ("stats", "range", "quant")[i % 3]
            self.ensure_gmm(dtype="f32" if a == "convert_gmm_f16" else None)
            self.ensure_gmm_plane(name)
            self.all_off()
            v = self.model.selected()
            if a == "init_gmm":   # new records: of the same dims, or of others
                g = self.new_gmm(like=v["spec"] if i % 2 == 0 else None)
                self.emit(op="init_gmm", gmm=g, z_base=0, nslices=g["dims"][2])
            elif a == "gmm_select":
                self.emit(op="gmm_select", slot=1 - self.model.slot)
            else:
                self.emit(op=a)
        else:   # the plane set baked slab by slab, each slab resident alone
            name, m = a, self.model
            if name == "range" and m.gmm_range is None:
                self.set_gmm_state("range")
            if name == "quant" and m.quant is None:
                self.set_gmm_state("quant")
            if m.gplanes[name] is not None:
                self.emit(op="release_gmm_" + GMM_NAME[name])
            g = self.new_gmm()
            nz = g["dims"][2]
            cuts = [0, int(self.rng.integers(1, nz)), nz]
            if nz >= 6 and i % 2:
                cuts = [0, nz // 3, 2 * nz // 3, nz]
            for z0, z1 in zip(cuts, cuts[1:]):
                self.emit(op="init_gmm", gmm=g, z_base=z0, nslices=z1 - z0)
                self.emit(op="bake_gmm_" + GMM_NAME[name])

    # ---- the caller's state between the scenes ----

    def any_plane(self):
        m = self.model
        return [s for s in SOURCES if m.plane_resident(s)], \
            [k for k, p in m.gplanes.items() if p is not None and all(s is not None for s in p["src"])]

    def ensure_any_plane(self):
        rec, gm = self.any_plane()
        if rec or gm:
            return
        if self.model.vol is not None or self.model.codec is not None:
            self.emit(op="bake_stats")
        elif self.model.selected() is not None:
            self.ensure_gmm_plane("stats")

    def table_spec(self, two=False):
        rng = self.rng
        kind = rc.TABLE_KINDS[int(rng.integers(0, 3))]
        shape = rc.TF2_SHAPES[int(rng.integers(0, len(rc.TF2_SHAPES)))] if two else \
            (rc.TF_SIZES[int(rng.integers(0, len(rc.TF_SIZES)))],)
        return dict(shape=tuple(shape), kind=kind, seed=int(rng.integers(1, 1 << 20)))

    def all_off(self):
        m = self.model
        if m.light:
            self.emit(op="set_light", light=None)
        if m.proj:
            self.emit(op="set_projection", mode=None)
        if m.tf:
            self.emit(op="set_transfer_function", table=None)
        if m.tf2:
            self.emit(op="set_transfer_function_2d", table=None, mv=0, voff=0.0, vscale=1.0)

    def set_tf2(self):
        """a 2-D table whose v plane is resident, of the family of the planes there are"""
        rng, m = self.rng, self.model
        rec, gm = self.any_plane()
        if rec:
            mv = int(rec[int(rng.integers(0, len(rec)))])
            if m.grad.get(mv) and rng.integers(0, 2):
                mv += G
            family = plane_family(mv)
        elif gm:
            mv, family = int(GMM_SETS[gm[int(rng.integers(0, len(gm)))]][0]), "gmm"
        else:
            mv, family = 2, "records"
        voff, vscale = rc.draw_window(rng, m.stat_of(family, mv))
        self.emit(op="set_transfer_function_2d", table=self.table_spec(True), mv=mv, voff=voff,
                  vscale=vscale)

    def stream_scene(self, kind):
        """The device copy of a table (kind: "tf" or "tf2") refreshed across a change of
        stream: a frame under it on this stream, the other table, the stream changed (its
        probe is the other table's frame), the table set anew -- the frame after that uploads
        a dirty copy that another stream read last (vr.h, vr_set_stream and
        vr_set_transfer_function: "the device copy is made or refreshed by the next frame
        that uses it").  A plane is resident throughout, so every probe is a table frame."""
        if self.model.vol is None and self.model.codec is None and self.model.selected() is None:
            self.ensure_gmm() if self.flavour == "gmm" else self.ensure_records()
        self.ensure_any_plane()
        self.all_off()
        one = (lambda: self.emit(op="set_transfer_function", table=self.table_spec()))
        first, other = (one, self.set_tf2) if kind == "tf" else (self.set_tf2, one)
        first()
        other()
        self.emit(op="set_stream", which=1 - self.model.stream)
        first()

    def sprinkle(self, b=False):
        if b:
            what = SPRINKLES_B[self.sprinkle_b % len(SPRINKLES_B)]
            self.sprinkle_b += 1
        else:
            what = SPRINKLES[self.sprinkle_at % len(SPRINKLES)]
            self.sprinkle_at += 1
        rng, m = self.rng, self.model
        if m.vol is None and m.codec is None and m.selected() is None:   # something to render
            self.ensure_gmm() if self.flavour == "gmm" else self.ensure_records()
        if what == "tf on":
            self.emit(op="set_transfer_function", table=self.table_spec())
        elif what == "all off":
            self.all_off()
        elif what == "tf off":
            self.emit(op="set_transfer_function", table=None)
        elif what == "tf2 off":
            self.emit(op="set_transfer_function_2d", table=None, mv=0, voff=0.0, vscale=1.0)
        elif what == "tf2 on":
            self.set_tf2()
        elif what == "light on":
            self.emit(op="set_light", light=rc.LIT_LIGHTS[int(rng.integers(0, 24))])
        elif what == "light off":
            self.emit(op="set_light", light=None)
        elif what == "proj on":
            self.emit(op="set_projection", mode=PROJECTIONS[int(rng.integers(0, 3))])
        elif what == "proj off":
            self.emit(op="set_projection", mode=None)
        elif what.startswith("budget"):
            self.emit(op="set_layout_budget", bytes=0 if what.endswith("0") else None)
        elif what == "knob":
            k, v = KNOBS[int(rng.integers(0, len(KNOBS)))]
            self.emit(op="set_tuning", key=k, value=v)
        else:
            for k in list(m.knobs) or [KNOBS[0][0]]:
                self.emit(op="set_tuning", key=k, value=None)

    # ---- bad calls: arguments the header refuses; the state stays as it was ----

    def bad_call(self):
        m, rng = self.model, self.rng
        nb = m.vol["nb"] if m.vol else 8
        for _ in range(len(BAD)):
            kind = BAD[(3 * self.seed + self.nbad) % len(BAD)]
            self.nbad += 1
            op = None
            if kind == "quantile":
                op = dict(op="set_quantile", q=(1.5, -0.25, math.nan)[self.nbad % 3])
            elif kind == "range nan":
                op = dict(op="set_query_range", lo=math.nan, hi=0.5, n=nb)
            elif kind == "table 257":
                op = dict(op="set_transfer_function", table=dict(shape=(257,), kind="unit", seed=7))
            elif kind == "bake without state":
                for q in QUERIES:
                    if m._query_ready(q) != OK:
                        op = dict(op="bake_" + QUERY_NAME[q])
            elif kind == "spread order":
                op = dict(op="set_quantile_spread", lo=0.75, hi=0.25)
            elif kind == "weights 3":
                op = dict(op="set_bin_weights", w=dict(kind="seeded", wseed=5, n=3))
            elif kind == "gmm range order":
                op = dict(op="set_gmm_range", lo=0.75, hi=0.25)
            elif kind == "light negative":
                op = dict(op="set_light", light=(0.5, -0.25, 0.0, 2))
            elif kind == "projection 4":
                op = dict(op="set_projection", mode=4)
            elif kind == "tf2 method 7":
                op = dict(op="set_transfer_function_2d", table=self.table_spec(True), mv=7,
                          voff=0.0, vscale=1.0)
            elif kind == "isovalue nan":
                op = dict(op="set_isovalue", theta=math.nan, n=nb)
            elif kind == "gradient 7":
                op = dict(op="bake_gradient", m=7)
            elif kind == "gradient without source":
                missing = [s for s in SOURCES if not m.plane_resident(s)]
                if missing:
                    op = dict(op="bake_gradient", m=int(missing[int(rng.integers(0, len(missing)))]))
            elif kind == "metric 5":
                op = dict(op="set_query_target", h=[1.0 / nb] * nb, metric=5, similarity=False)
            elif kind == "slot 2":
                op = dict(op="gmm_select", slot=2)
            elif kind == "convert twice":
                if m.vol is None or m.vol["dtype"] == "f16" or m.vol["narrowed"]:
                    op = dict(op="convert_f16")
            elif kind == "region outside":
                d = m.vol["dims"] if m.vol else (4, 4, 4)
                op = dict(op="set_query_target_region", lo=(0, 0, 0), hi=(d[0] + 1, 1, 1),
                          metric="l1", similarity=False)
            elif kind == "gmm range nan":
                op = dict(op="set_gmm_range", lo=math.nan, hi=1.0)
            elif kind == "bake gmm without state":
                if m.selected() is None:
                    op = dict(op="bake_gmm_stats")
                elif m.gmm_range is None:
                    op = dict(op="bake_gmm_range")
                elif m.quant is None:
                    op = dict(op="bake_gmm_quantile")
            elif kind == "table nan":
                op = dict(op="set_transfer_function", table=self.table_spec(), poison=True)
            elif kind == "weights inf":
                op = dict(op="set_crossing_weights", w=dict(kind="seeded", wseed=9, n=nb),
                          poison=True)
            else:
                op = dict(op="set_transfer_function_2d",
                          table=dict(shape=(33, 32), kind="unit", seed=3), mv=2, voff=0.0, vscale=1.0)
            if op is not None:
                before = copy.deepcopy(m)
                self.emit(**op)
                assert (self.ops[-1]["status"] != OK and _same_state(before, m)), op
                return

    # ---- probes ----

    def candidates(self):
        """(entry, method) of every frame that can be asked for now"""
        m, out = self.model, []
        if m.vol is not None:
            out += [("render", k) for k in (1, 2, 3, 7, 10, 11, 12, 13)]
        if m.codec is not None:
            out += [("render", k) for k in (4, 5, 6)]
        out += [("render", G + s) for s in SOURCES if m.grad[s]]
        if m.selected() is not None:
            out += [("render_gmm", k) for k in (1, 2, 10, 11)]
        if any(p is not None for p in m.gplanes.values()):
            out += [("render_gmm_baked", k) for k in (1, 2, 10, 11, 13)]
        return out

    def frame(self, entry, method, tiny_ok=True):
        rng, m = self.rng, self.model
        W, H = int(rng.integers(1, FRAME_MAX[0] + 1)), int(rng.integers(1, FRAME_MAX[1] + 1))
        tiny = tiny_ok and rng.integers(0, 16) == 0
        if tiny:
            W, H = 1, 1
        if W * H < 16:   # a few rays: from inside the volume, so that they hit
            kind, rot, tr = rc.draw_view(rng, 2)
        else:
            kind, rot, tr = rc.draw_view(rng)
        family = "gmm" if entry != "render" else plane_family(method) or "records"
        params = rc.draw_params(rng, m.stat_of(family, method))
        return dict(entry=entry, method=method, W=W, H=H, kind=kind, rotation=rot, translation=tr,
                    params=params)

    def deal_probe(self, op):
        """a frame the library must serve now, one that reads what the op touched if any does"""
        cands = self.candidates()
        if not cands:
            return None
        order = self.rng.permutation(len(cands))
        family, first, second = TOUCHES.get(op["op"], (None, (), ()))
        if op["op"] in ("bake_gradient", "release_gradient"):
            family, first, second = plane_family(op["m"]), (G + op["m"],), (op["m"],)

        def rank(c):
            mine = "gmm" if c[0] != "render" else plane_family(c[1]) or "records"
            if family is not None and mine != family:
                return 2
            return 0 if c[1] in first else 1 if c[1] in second else 2
        cands = sorted((cands[i] for i in order), key=rank)
        for entry, method in cands:
            if "status" not in self.model.expect(dict(entry=entry, method=method)):
                return self.frame(entry, method)
        return None

    def deal_refusal(self):
        """a frame the library must refuse now, a precedence pair first"""
        m = self.model
        missing = [s for s in SOURCES if not m.grad[s]]
        cands = self.candidates() + [("render", G + s) for s in missing[:1]] + \
            [("render", 1), ("render", 4), ("render_gmm", 1), ("render_gmm", 13),
             ("render_gmm_baked", 12), ("render_gmm_baked", 1), ("render_gmm_baked", 11)]
        order = self.rng.permutation(len(cands))
        found = None
        for i in order:
            entry, method = cands[i]
            e = m.expect(dict(entry=entry, method=method))
            if "status" not in e:
                continue
            if " over " in e["why"]:
                found = (entry, method, e)
                break
            found = found or (entry, method, e)
        if found is None:
            return None
        entry, method, e = found
        f = self.frame(entry, method, tiny_ok=False)
        return dict(f, status=e["status"], why=e["why"])

    def deal_stat(self):
        """plane_range or plane_histogram on a resident record or codec plane"""
        m, rng = self.model, self.rng
        have = [s for s in SOURCES if m.plane_resident(s)]
        have += [G + s for s in SOURCES if m.grad[s]]
        if not have:
            return None
        u = int(have[int(rng.integers(0, len(have)))])
        family = plane_family(u)
        dims = m.vol["dims"] if family == "records" else m.codec["dims"]
        box = None
        if rng.integers(0, 2):
            spans = [rc._span(rng, n) for n in dims]
            box = tuple(int(v) for s in spans for v in s)
        if rng.integers(0, 2):
            return dict(call="plane_range", u=u, box=box)
        mates = [v for v in have if plane_family(v) == family]
        v = int(mates[int(rng.integers(0, len(mates)))]) if rng.integers(0, 2) else None
        nu, nv = (int(rng.integers(1, 33)), int(rng.integers(1, 17))) if v else \
            (int(rng.integers(1, 257)), 1)
        return dict(call="plane_histogram", u=u, v=v, nu=nu, nv=nv, box=box,
                    wu=rc.draw_window(rng, m.stat_of(family, u)),
                    wv=rc.draw_window(rng, m.stat_of(family, v)) if v else None)


GMM_NAME = {"stats": "stats", "range": "range", "quant": "quantile"}
# op -> (family, the methods whose frames read what it touches): a probe prefers them, the
# first group before the second (the windows of variance and entropy miss more often)
_RECORDS = ("records", (1, 7, 10, 11, 12, 13), (2, 3))
TOUCHES = {"init_distribution": _RECORDS, "convert_f16": _RECORDS,
           "init_codec": ("codec", (4, 5, 6), ()), "bake_stats": ("records", (1, 7), (2, 3)),
           "release_stats": _RECORDS,
           "init_gmm": ("gmm", (1, 10, 11), (2,)), "convert_gmm_f16": ("gmm", (1, 10, 11), (2,)),
           "gmm_select": ("gmm", (1, 10, 11), (2,)),
           "bake_gmm_stats": ("gmm", (1,), (2,)), "release_gmm_stats": ("gmm", (1,), (2,)),
           "bake_gmm_range": ("gmm", (10, 13), ()), "release_gmm_range": ("gmm", (10, 13), ()),
           "set_gmm_range": ("gmm", (10, 13), ()), "clear_gmm_range": ("gmm", (10, 13), ()),
           "bake_gmm_quantile": ("gmm", (11,), ()), "release_gmm_quantile": ("gmm", (11,), ())}
for _m, _n in QUERY_NAME.items():
    TOUCHES["bake_" + _n] = TOUCHES["release_" + _n] = ("records", (_m,), ())
for _op in ("set_bin_weights", "set_query_range", "clear_bin_weights"):
    TOUCHES[_op] = ("records", (10,), ())
for _op in ("set_quantile", "set_quantile_spread", "clear_quantile"):
    TOUCHES[_op] = (None, (11,), ())   # (the records' and the GMM volumes')
for _op in ("set_query_target", "set_query_target_region", "clear_query_target"):
    TOUCHES[_op] = ("records", (12,), ())
for _op in ("set_isovalue", "set_crossing_weights", "clear_crossing_weights"):
    TOUCHES[_op] = ("records", (13,), ())

# the op vocabulary: the public state-changing API (api.py's names; a clear_* of the record
# queries is the setter called with None)
OPS = ("init_distribution", "convert_f16", "init_codec", "freeCudaBuffers", "init_gmm", "free_gmm",
       "gmm_select", "convert_gmm_f16", "bake_stats", "release_stats", "bake_weighted",
       "release_weighted", "bake_quantile", "release_quantile", "bake_distance",
       "release_distance", "bake_crossing", "release_crossing", "bake_gradient",
       "release_gradient", "bake_gmm_stats", "release_gmm_stats", "bake_gmm_range",
       "release_gmm_range", "bake_gmm_quantile", "release_gmm_quantile", "set_bin_weights",
       "clear_bin_weights", "set_query_range", "set_quantile", "set_quantile_spread",
       "clear_quantile", "set_query_target", "clear_query_target", "set_query_target_region",
       "set_isovalue", "set_crossing_weights", "clear_crossing_weights", "set_gmm_range",
       "clear_gmm_range", "set_transfer_function", "set_transfer_function_2d", "set_projection",
       "set_light", "set_stream", "set_layout_budget", "set_tuning")
assert all(hasattr(Model, "_" + _op) for _op in OPS)


def _same_state(a, b):
    skip = ("arrays", "layout_zero")
    return repr(sorted((k, repr(v)) for k, v in a.__dict__.items() if k not in skip)) == \
        repr(sorted((k, repr(v)) for k, v in b.__dict__.items() if k not in skip))


def _scenes(seed):
    """the scenes of a session, dealt in turn so that 48 sessions go round every list
    several times: the 36 sessions that hold records share 48 own events and 30 volume
    scenes, the 24 that hold a GMM volume 72 GMM scenes"""
    flavour, t = FLAVOURS[seed % 4], seed // 4
    own, vol = (lambda i: (("own", None, None), i)), (lambda i: (("volume", None, None), i))
    cod = lambda i: (("codec", None, None), i)
    gm = lambda i: (GMM_SCENES[i % len(GMM_SCENES)], i)
    if flavour == "records":
        return [own(2 * t), vol(t), own(2 * t + 1)]
    if flavour == "records+codec":
        return [cod(t), own(24 + t), vol(12 + t)]
    if flavour == "gmm":
        return [gm(4 * t + j) for j in range(4)]
    return [own(36 + t), gm(48 + 2 * t)] + ([vol(24 + t // 2)] if t % 2 == 0 else []) + \
        [gm(48 + 2 * t + 1)]


def session(seed):
    """the session of a seed: dict(seed, flavour, first, ops)"""
    g = _Gen(seed)
    first = g.first()
    try:
        if g.layout:
            g.layout_scene()
        for scene, count in _scenes(seed):
            g.scene(scene, count)
        if g.flavour == "mixed" and g.turn % 2:
            g.reshape_scene()
        if len(g.ops) <= 14:   # (ten sessions and more have the room)
            g.stream_scene(("tf", "tf2")[(seed + seed // 4) % 2])
        g.sprinkle(b=True)
        while len(g.ops) < 16:
            g.sprinkle(b=True)
    except _Full:
        pass
    return dict(seed=seed, flavour=g.flavour, first=first, ops=g.ops)
