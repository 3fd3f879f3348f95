"""CPU census of the session sweep (tests/session_cases.py, run on the GPU by
tests/test_gpu_sessions.py): the generator, the model and the references only, and the
model's host-state half against libvr.so, which needs no device for it.  It holds the
helpers that turn an op into library calls, the library's getters into a census and a
probe's recipe into its reference frame, which the GPU test imports.

What it proves, so that the GPU sweep is worth running:

  sessions are reproducible, printable and inside the library's documented limits;
  over the 48 sessions every op of the vocabulary occurs at least 4 times, every (plane
  family, documented cause of its drop) pair of session_cases.DROPS at least twice with
  the plane resident, the model drops a plane on no other op, every precedence pair is
  probed as a refusal, new contents of the same shape arrive with planes resident at
  least 12 times and records of another shape at least 4 times;
  every change of stream is followed by a served table, projection or lit frame, and both
  tables are refreshed at least 3 times while the stream that last read them is another
  (table_upload's flags, restated);
  of the steps that leave a record or codec plane resident, one in four calls plane_range
  or plane_histogram;
  the probes see the changes: of the probes that follow new contents of the same shape, a
  conversion to f16, a rebake after a changed query state or a changed table, light or
  projection, at most one in eight shows the same words under the state before the change
  (a stale plane, copy or table would render exactly that frame);
  every function include/vr.h exports is an op, a getter of the census, a call of the
  probes or listed in NOT_SWEPT with its reason;
  the host-state setters of every session, replayed against the library without a GPU,
  leave its getters where the model says.

The census as it stands (printed by the tests): 48 sessions of 16-20 ops, 1 144 steps with
the first volumes and their query state, 78 of them bad calls, 962 served and 1 144 refused
probes dealt (166 of them frames to which two statuses apply), 13 uploads of the same shape
and 6 of another over resident planes, 13 changes of stream with 5 (1-D) and 6 (2-D) stale
tables refreshed across them, 134 plane_range / plane_histogram calls over 414 steps with a
plane to call them on; blind probes 3 of 182 (new contents 0/14, f16 conversion 0/9, rebake
1/16, table, light or projection 2/143); 438 host-state calls replayed against the library,
56 of them refused.  The file takes 14 s.
"""
import collections
import copy
import math
import os
import re

import numpy as np
import pytest

import random_cases as rc
import ref_crossing
import ref_distance
import ref_gmm_quantile
import ref_gmm_range
import ref_gradient
import ref_histogram as rh
import ref_numpy
import ref_projection
import ref_quantile
import ref_shading
import ref_transfer
import ref_transfer2
import ref_weighted
import session_cases as sc
from test_random_cases import blend_of, camera, gmm_consts, gmm_oracle_plane

G = sc.G
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- specs -> arrays ----

class Arrays:
    """the arrays of the sessions' volume specs, and the planes numpy makes of them, kept"""

    def __init__(self, orc):
        self.orc = orc
        self.kept = {}

    def _keep(self, key, make):
        if key not in self.kept:
            self.kept[key] = make()
        return self.kept[key]

    def upload(self, spec):
        """the records init_distribution takes: float32, or float16"""
        def make():
            v = self.orc.synth_volume(*spec["dims"], spec["nb"], seed=spec["seed"])
            return v.astype(np.float16) if spec["dtype"] == "f16" else v
        return self._keep(("upload", tuple(spec["dims"]), spec["nb"], spec["dtype"], spec["seed"]),
                          make)

    def records(self, spec):
        """the records resident: the upload, narrowed where convert_f16 did so (round to
        nearest even, subnormals kept: numpy's astype)"""
        v = self.upload(spec)
        return v.astype(np.float16) if spec.get("narrowed") else v

    def codec(self, spec):
        return self._keep(("codec", tuple(spec["dims"]), spec["nb"], spec["seed"]),
                          lambda: self.orc.synth_codec(*spec["dims"], spec["nb"], seed=spec["seed"]))

    def gmm(self, spec):
        """(the planes init_gmm takes, the float32 records the references decode)"""
        def make():
            wm, sg = self.orc.synth_gmm(*spec["dims"], spec["K"], seed=spec["seed"])
            if spec["dtype"] == "f16":
                wm, sg = wm.astype(np.float16), sg.astype(np.float16)
            return wm, sg
        up = self._keep(("gmm", tuple(spec["dims"]), spec["K"], spec["dtype"], spec["seed"]), make)
        half = spec["dtype"] == "f16" or spec.get("narrowed")
        wide = tuple(a.astype(np.float16).astype(np.float32) if half else a for a in up)
        return up, wide


def new_model(arrays):
    m = sc.Model()
    m.arrays = arrays
    return m


# ---- an op -> the library ----

HOST_OPS = ("set_bin_weights", "clear_bin_weights", "set_query_range", "set_quantile",
            "set_quantile_spread", "clear_quantile", "set_query_target", "clear_query_target",
            "set_isovalue", "set_crossing_weights", "clear_crossing_weights", "set_gmm_range",
            "clear_gmm_range", "set_transfer_function", "set_transfer_function_2d",
            "set_projection", "set_light")


def apply_op(pkg, op, arrays, dev=None):
    """the library calls of an op (api.py's functions); dev: the GPU test's torch, second
    stream and the tensor an adopted volume lives in"""
    name = op["op"]
    if name == "init_distribution":
        a = arrays.upload(op["vol"])
        if op["vol"]["adopt"]:
            dev.adopted = dev.torch.from_numpy(a).cuda()
            pkg.init_distribution(dev.adopted, adopt=True)
        else:
            pkg.init_distribution(a)
    elif name == "init_codec":
        pkg.init_codec(*arrays.codec(op["codec"]))
    elif name == "init_gmm":
        (wm, sg), _ = arrays.gmm(op["gmm"])
        z0, z1 = op["z_base"], op["z_base"] + op["nslices"]
        pkg.init_gmm(wm[z0:z1], sg[z0:z1], op["gmm"]["dims"], z_base=z0)
    elif name in ("set_bin_weights", "set_crossing_weights"):
        w = sc.weights_value(op["w"]).copy()
        if op.get("poison"):
            w[-1] = np.inf
        getattr(pkg, name)(w)
    elif name.startswith("clear_") and name != "clear_gmm_range":
        {"clear_bin_weights": pkg.set_bin_weights, "clear_quantile": pkg.set_quantile,
         "clear_query_target": pkg.set_query_target,
         "clear_crossing_weights": pkg.set_crossing_weights}[name](None)
    elif name == "set_query_range":
        pkg.set_query_range(op["lo"], op["hi"], op["n"])
    elif name == "set_quantile":
        pkg.set_quantile(op["q"])
    elif name == "set_quantile_spread":
        pkg.set_quantile_spread(op["lo"], op["hi"])
    elif name == "set_query_target":
        pkg.set_query_target(np.array(op["h"], np.float32), op["metric"], op["similarity"])
    elif name == "set_query_target_region":
        pkg.set_query_target_region(op["lo"], op["hi"], metric=op["metric"],
                                    similarity=op["similarity"])
    elif name == "set_isovalue":
        pkg.set_isovalue(op["theta"], op["n"])
    elif name == "set_gmm_range":
        pkg.set_gmm_range(op["lo"], op["hi"])
    elif name == "set_transfer_function":
        t = op["table"]
        pkg.set_transfer_function(None if t is None else sc.table_value(t, op.get("poison")))
    elif name == "set_transfer_function_2d":
        t = op["table"]
        if t is None:
            pkg.set_transfer_function_2d(None)
        else:
            pkg.set_transfer_function_2d(sc.table_value(t, op.get("poison")), op["mv"], op["voff"],
                                         op["vscale"])
    elif name == "set_projection":
        pkg.set_projection(op["mode"])
    elif name == "set_light":
        lt = op["light"]
        pkg.set_light(None) if lt is None else pkg.set_light(lt[0], lt[1], lt[2], 1 << lt[3])
    elif name == "set_stream":
        pkg.set_stream(dev.stream if op["which"] else None)
    elif name == "set_layout_budget":
        pkg.set_layout_budget(op["bytes"])
    elif name == "set_tuning":
        pkg.set_tuning(op["key"], op["value"])
    elif name in ("bake_gradient", "release_gradient"):
        getattr(pkg, name)(op["m"])
    elif name == "gmm_select":
        pkg.gmm_select(op["slot"])
    else:   # convert_f16, freeCudaBuffers, free_gmm, convert_gmm_f16, every other bake and release
        getattr(pkg, name)()


def apply_and_check(pkg, op, arrays, dev=None):
    """apply the op; a bad call must raise VRError with the model's status"""
    if op["status"] == sc.OK:
        apply_op(pkg, op, arrays, dev)
        return
    with pytest.raises(pkg.VRError) as e:
        apply_op(pkg, op, arrays, dev)
    assert e.value.status == op["status"], (op, e.value.status, str(e.value))
    pkg._lib.load().vr_clear_error()


# ---- the library's getters -> a census ----

VALUE_KEYS = ("bin_weights", "quantile", "query_target", "crossing_weights", "gmm_range",
              "transfer_function", "transfer_function_2d", "projection", "light")


def _or_none(pkg, getter):
    """a getter that is VR_ERR_STATE while nothing is set"""
    try:
        return getter()
    except pkg.VRError as e:
        assert e.status == sc.ERR_STATE, str(e)
        pkg._lib.load().vr_clear_error()
        return None


def library_census(pkg, host_only=False):
    """Model.census()'s dict as the library reports it; host_only: the value getters"""
    c = {"bin_weights": _or_none(pkg, pkg.bin_weights), "quantile": _or_none(pkg, pkg.quantile),
         "query_target": _or_none(pkg, pkg.query_target),
         "crossing_weights": _or_none(pkg, pkg.crossing_weights),
         "gmm_range": _or_none(pkg, pkg.gmm_range), "transfer_function": pkg.transfer_function(),
         "transfer_function_2d": pkg.transfer_function_2d(), "projection": pkg.projection(),
         "light": pkg.light()}
    if host_only:
        return c
    raw, codec = pkg.stats_info()
    for name, info in (("gmm_stats_info", pkg.gmm_stats_info), ("gmm_range_info", pkg.gmm_range_info),
                       ("gmm_quantile_info", pkg.gmm_quantile_info)):
        _, ptr, _, nbaked = info()
        c[name] = (bool(ptr), nbaked)
    c.update({
        "weighted_info": bool(pkg.weighted_info()[0]), "quantile_info": bool(pkg.quantile_info()[0]),
        "distance_info": bool(pkg.distance_info()[0]), "crossing_info": bool(pkg.crossing_info()[0]),
        "gradient_info": {m: bool(pkg.gradient_info(m)[0]) for m in sc.SOURCES},
        "stats_info": (bool(raw[0]), bool(codec[0])),
        "volume_dtype": _or_none(pkg, pkg.volume_dtype), "gmm_dtype": _or_none(pkg, pkg.gmm_dtype),
        "layout_zero": pkg.layout_info()["resident_bytes"] == 0})
    return c


def _equal(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and np.asarray(a).shape == np.asarray(b).shape \
            and np.array_equal(np.asarray(a, np.float32).view(np.uint32),
                               np.asarray(b, np.float32).view(np.uint32))
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    return a == b


def census_differences(got, want):
    """the keys on which the library's census differs from the model's.  layout_zero is
    held only where the model says that no copy can be resident."""
    out = []
    for k, w in want.items():
        if k not in got or (k == "layout_zero" and not w):
            continue
        if not _equal(got[k], w):
            out.append(f"{k}: library {got[k]!r}, model {w!r}")
    return out


# ---- a probe's recipe -> its reference frame ----

def _record_plane(arrays, model, m):
    vol = arrays.records(model.vol)
    wide = np.asarray(vol).astype(np.float32)
    with np.errstate(all="ignore"):
        if m in (1, 2, 3):
            return ref_numpy.stat(wide, m - 1)
        if m == 10:
            return ref_weighted.lin_stat(wide, sc.weights_value(model.weights))
        if m == 11:
            lo, hi, spread = model.quant
            return ref_quantile.quantile_stat(wide, (lo, hi) if spread else lo)
        if m == 12:
            t = model.target
            return ref_distance.distance_stat(wide, np.array(t["h"], np.float32), t["metric"],
                                              t["similarity"])
    return ref_crossing.cdf_plane(vol, sc.weights_value(model.xweights))


def _gmm_records_plane(pkg, orc, arrays, model, spec, m, device_plane=None):
    """the statistic m of every voxel of the GMM records `spec` under the model's state"""
    wm, sg = arrays.gmm(spec)[1]
    table, steps = gmm_consts(pkg)
    with np.errstate(all="ignore"):
        if m in (10, 13):
            lo, hi = model.gmm_range
            return ref_gmm_range.range_stat(wm, sg, lo, hi, table)
        if m == 11:
            lo, hi, spread = model.quant
            return ref_gmm_quantile.quantile_stat(wm, sg, lo, hi, spread, table, steps)
    return gmm_oracle_plane(orc, (wm, sg), m)


def plane_of(pkg, orc, arrays, model, family, m, device_plane=None):
    """the baked plane of method m (32 + m: its gradient plane) as numpy computes it from
    the model's current records and state, (nz, ny, nx) float32.  A GMM plane set is put
    together slice by slice from the records each slice was baked from; device_plane(m):
    the GPU test's read-back of a GMM mean or variance plane, which has no bit-exact
    restatement (tests/test_gpu_random_transfer.py)."""
    if m > G:
        return ref_gradient.gradient_plane(plane_of(pkg, orc, arrays, model, family, m - G))[0]
    if family == "records":
        key = ("plane", repr(model.vol), m, repr((model.weights, model.quant, model.target,
                                                  model.xweights)[m - 10]) if m >= 10 else None)
        return arrays._keep(key, lambda: _record_plane(arrays, model, m))
    if family == "codec":
        dec = arrays._keep(("decoded", repr(model.codec)),
                           lambda: ref_numpy.codec_decode(*arrays.codec(model.codec)))
        with np.errstate(all="ignore"):
            return ref_numpy.codec_stat(dec, m - 4)
    if m <= 2 and device_plane is not None:
        return device_plane(m)
    p = model.gplanes[model._gmm_set(m)]
    state = repr((model.gmm_range, model.quant))
    out = None
    for z, spec in enumerate(p["src"]):
        full = arrays._keep(("gmm plane", repr(spec), m, state),
                            lambda: _gmm_records_plane(pkg, orc, arrays, model, spec, m))
        out = np.zeros_like(full) if out is None else out
        out[z] = full[z]
    return out


def reference(pkg, orc, arrays, model, probe, recipe, device_plane=None):
    """(RGBA8, float RGBA, samples) of the probe by the recipe of model.expect(probe)"""
    W, H, kw = probe["W"], probe["H"], dict(probe["params"])
    cam = camera(pkg, probe)
    family, route, u, v = recipe["family"], recipe["route"], recipe["u"], recipe["v"]
    params = lambda **more: orc.make_params(W, H, cam, density=kw["density"],
                                            brightness=kw["brightness"], transfer_offset=kw["toff"],
                                            transfer_scale=kw["tscale"], query_method=u, **more)
    if recipe["bar"] == "parity":   # the oracle: methods 1/2/3/7 and the codec's 4/5/6
        if family == "codec":
            return orc.render_codec(*arrays.codec(model.codec), params())[:3]
        wide = np.asarray(arrays.records(model.vol)).astype(np.float32)
        return orc.render(wide, params(m7_dims=tuple(model.vol["dims"])))[:3]
    if route == "march" and family == "gmm":   # the records resident in the selected slot
        spec = model.selected()["spec"]
        if recipe["bar"] == "gmm":
            wm, sg = arrays.gmm(spec)[1]
            r = orc.render_gmm(wm, sg, spec["dims"], params())
            return r["out"], r["out_f"], r["out_n"]
        F = _gmm_records_plane(pkg, orc, arrays, model, spec, u)
        return ref_crossing.render_plane(F, W, H, cam, blend=ref_crossing.trilinear, **kw)
    P = {k: plane_of(pkg, orc, arrays, model, family, k, device_plane)
         for k in (u, v) if k is not None}
    table = None if model.tf is None else sc.table_value(model.tf)
    if route in ("march", "plane"):
        return ref_crossing.render_plane(P[u], W, H, cam, blend=blend_of(u), **kw)
    if route == "tf":
        return ref_transfer.render_plane(P[u], W, H, cam, table, blend=blend_of(u), **kw)
    if route == "tf2":
        t2 = model.tf2
        return ref_transfer2.render_planes(P[u], P[v], W, H, cam, sc.table_value(t2["table"]),
                                           blend_u=blend_of(u), blend_v=blend_of(v),
                                           voff=t2["voff"], vscale=t2["vscale"], **kw)
    if route == "proj":
        return ref_projection.render_plane(P[u], W, H, cam, model.proj, table, blend=blend_of(u),
                                           brightness=kw["brightness"], toff=kw["toff"],
                                           tscale=kw["tscale"])
    assert route == "lit", recipe
    return ref_shading.render_plane(P[u], W, H, cam, table, model.light, blend=blend_of(u), **kw)


def stat_reference(pkg, orc, arrays, model, stat):
    """what plane_range or plane_histogram must return for a session's `stat` call"""
    family = sc.plane_family(stat["u"])
    pu = plane_of(pkg, orc, arrays, model, family, stat["u"])
    if stat["call"] == "plane_range":
        return rh.plane_range(pu, stat["box"])
    pv = None if stat["v"] is None else plane_of(pkg, orc, arrays, model, family, stat["v"])
    return rh.histogram(pu, stat["nu"], stat["wu"], pv, stat["nv"], stat["wv"] or (0.0, 1.0),
                        stat["box"])


# ---- the census ----

@pytest.fixture(scope="module")
def sessions():
    return [sc.session(seed) for seed in range(sc.N_SESSIONS)]


def steps(session):
    return session["first"] + session["ops"]


def test_sessions_are_reproducible_and_in_bounds(sessions):
    for seed, s in enumerate(sessions):
        assert s == sc.session(seed) and s["seed"] == seed and s["flavour"] == sc.FLAVOURS[seed % 4]
        assert s == eval(repr(s), {"inf": math.inf, "nan": math.nan}) or \
            "nan" in repr(s)   # printable: a failure shows it whole (a NaN equals nothing)
        assert 12 <= len(s["ops"]) <= 20, (seed, len(s["ops"]))
        for op in steps(s):
            assert op["op"] in sc.OPS
            if "vol" in op:
                d, nb = op["vol"]["dims"], op["vol"]["nb"]
                assert nb in rc.INSTANCE_BINS and 2 <= min(d) and d[1] <= 24 and d[2] <= 24
                assert d[0] <= 24 or d[0] in rc.EDGE_NX
            if "gmm" in op:
                assert all(2 <= n <= 16 for n in op["gmm"]["dims"]) and op["gmm"]["K"] in (8, 16, 32)
            if op["status"] == sc.OK and op.get("table"):
                shape = op["table"]["shape"]
                assert int(np.prod(shape)) <= (rc.make_table(op["table"]).size // 4) <= 1024
                assert max(shape) <= 256
            for f in (op["probe"], op["refuse"]):
                if f is not None:
                    assert 1 <= f["W"] <= sc.FRAME_MAX[0] and 1 <= f["H"] <= sc.FRAME_MAX[1]
                    assert 0.005 <= f["params"]["density"] <= 0.5001
                    assert math.isfinite(f["params"]["toff"]) and f["params"]["tscale"] != 0


def _resident(model):
    """{plane family: resident}"""
    out = {"stats": model.stats, "cstats": model.cstats}
    out.update({sc.QUERY_FAMILY[m]: model.qplane[m] for m in sc.QUERIES})
    out.update({f"gradient {m}": model.grad[m] for m in sc.SOURCES})
    out.update({f"gmm {k}": p is not None for k, p in model.gplanes.items()})
    return out


def test_every_op_and_cause_occurs(sessions):
    ops, causes, undocumented = collections.Counter(), collections.Counter(), []
    refusals, reuploads, served, refused, bad, nsteps = collections.Counter(), 0, 0, 0, 0, 0
    reshaped = stats = record_steps = several = 0
    streams, cross = [], collections.Counter()
    for s in sessions:
        model = sc.Model()
        # table_upload's state (vr_api.cpp): per device table whether a copy exists, whether
        # it is stale, and the stream of the last upload or frame that touched it
        tables = {k: dict(dev=False, dirty=False, last=None) for k in ("tf", "tf2", "rtf")}
        with_plane = mine = 0
        for op in steps(s):
            before, vol = _resident(model), copy.deepcopy(model.vol)
            assert model.apply(op) == op["status"], op   # the dict carries the model's own answer
            after = _resident(model)
            ops[op["op"]] += 1
            nsteps += 1
            bad += op["status"] != sc.OK
            for family, was in before.items():
                if not was or after[family]:
                    continue
                cause = op["op"]
                if family.startswith("gradient") and cause != "release_gradient":
                    m = int(family.split()[1])   # its source's plane went with it
                    assert not model.plane_resident(m), (family, op)
                    cause = "source went"
                causes[family, cause] += 1
                if cause not in sc.DROPS[family]:
                    undocumented.append((family, op))
            if op["op"] == "init_distribution" and vol is not None and any(before.values()):
                same = (tuple(vol["dims"]), vol["nb"]) == (tuple(op["vol"]["dims"]), op["vol"]["nb"])
                reuploads += same
                reshaped += not same
            if op["status"] == sc.OK:
                if op["op"] == "set_transfer_function" and op["table"] is not None:
                    tables["tf"]["dirty"] = True
                if op["op"] == "set_transfer_function_2d" and op["table"] is not None:
                    tables["tf2"]["dirty"] = True
                if op["op"] == "freeCudaBuffers":   # "frees only the device copy"
                    tables = {k: dict(dev=False, dirty=False, last=None) for k in tables}
            served += op["probe"] is not None
            route = None
            if op["probe"] is not None:
                recipe = model.expect(op["probe"])
                assert "status" not in recipe, op
                route = recipe["route"]
                if route in ("tf", "tf2", "proj", "lit"):   # the frame's table, as table_upload sees it
                    t = tables[route if route == "tf2" else "tf" if model.tf else "rtf"]
                    if not t["dev"]:
                        t.update(dev=True, dirty=True, last=model.stream)
                    if t["dirty"]:
                        cross["tf2" if route == "tf2" else "tf" if model.tf else "rtf"] += \
                            t["last"] != model.stream
                    t.update(dirty=False, last=model.stream)
            if op["op"] == "set_stream" and op["status"] == sc.OK:
                streams.append((s["seed"], route))
            # (plane_range and plane_histogram read record and codec planes, no GMM set)
            with_plane += any(r for f, r in after.items() if not f.startswith("gmm"))
            mine += op["stat"] is not None
            if op["stat"] is not None:
                assert model.plane_resident(op["stat"]["u"]), op
            if op["refuse"] is not None:
                e = model.expect(op["refuse"])
                assert e.get("status") == op["refuse"]["status"], op
                refused += 1
                several += e["several"]
                refusals[e["why"]] += 1
        # one step in four calls plane_range or plane_histogram, or the next one after it at
        # which a plane is resident: of the steps that leave one resident, one in four
        assert mine >= with_plane // 4, (s["seed"], mine, with_plane)
        stats, record_steps = stats + mine, record_steps + with_plane
    print(f"sessions: {nsteps} steps, {bad} bad calls, {served} served and {refused} refused "
          f"probes ({several} where two statuses apply), {reuploads} uploads of the same shape "
          f"and {reshaped} of another over resident planes, {stats} plane_range / plane_histogram "
          f"calls over {record_steps} steps that leave a record or codec plane resident, {len(streams)} changes of "
          f"stream, dirty tables uploaded across streams {dict(cross)}; refusals {dict(refusals)}")
    assert not undocumented, undocumented[:3]
    for op in sc.OPS:
        assert ops[op] >= 4, (op, ops[op])
    for family, documented in sc.DROPS.items():
        for cause in documented:
            assert causes[family, cause] >= 2, (family, cause, causes[family, cause])
    for pair in ("light over projection", "projection over 2-D table", "light over 2-D table"):
        assert refusals[pair] >= 2, (pair, refusals[pair])
    assert reuploads >= 12 and 4 <= reshaped <= reuploads, (reuploads, reshaped)
    # after every change of stream the probe is a table, projection or lit frame, and both
    # tables are refreshed with their last reader on the other stream
    assert len(streams) >= 8 and all(r in ("tf", "tf2", "proj", "lit") for _, r in streams), streams
    assert cross["tf"] >= 3 and cross["tf2"] >= 3, cross
    assert stats >= 100, stats
    assert several >= 20, several
    assert sum(s["ops"][0]["op"] == "set_tuning" and s["ops"][0]["probe"]["kind"] == 1
               for s in sessions) >= 6
    assert 8 * bad >= sum(len(s["ops"]) for s in sessions) // 2   # one op in about ten (1/16 .. )
    assert 2 * served >= nsteps, (served, nsteps)


# the probes must see the changes: the kinds of change, and for each the model state a
# stale plane, copy or table would be rendered from
STATE_OF = {"bake_weighted": "weights", "bake_quantile": "quant", "bake_distance": "target",
            "bake_crossing": "xweights", "bake_gmm_range": "gmm_range", "bake_gmm_quantile": "quant"}
TABLE_OPS = ("set_transfer_function", "set_transfer_function_2d", "set_light", "set_projection")


def _words_equal(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
               for x, y in zip((np.ascontiguousarray(v) for v in a),
                               (np.ascontiguousarray(v) for v in b)))


def test_changes_are_visible(pkg, orc, sessions):
    """at most one probe in eight is blind, over all sessions and within each kind of change"""
    arrays = Arrays(orc)
    blind, seen = collections.Counter(), collections.Counter()
    for s in sessions:
        model = new_model(arrays)
        baked_from = {}   # bake op -> the state its plane was last baked from
        for op in steps(s):
            before = copy.deepcopy(model)
            model.apply(op)
            name, probe, stale, kind = op["op"], op["probe"], None, None
            if op["status"] != sc.OK:
                continue
            if name == "init_distribution" and before.vol is not None and \
                    (tuple(before.vol["dims"]), before.vol["nb"]) == \
                    (tuple(model.vol["dims"]), model.vol["nb"]):
                kind, stale = "new contents", copy.deepcopy(model)
                stale.vol = before.vol
            elif name == "init_gmm" and before.selected() is not None and model.selected()["nzs"] == \
                    model.selected()["spec"]["dims"][2] and \
                    before.selected()["spec"]["dims"] == model.selected()["spec"]["dims"] and \
                    before.selected()["spec"]["K"] == model.selected()["spec"]["K"] and \
                    before.selected()["nzs"] == model.selected()["nzs"]:
                kind, stale = "new contents", copy.deepcopy(model)
                stale.gmm[stale.slot] = before.selected()
            elif name == "convert_f16":
                kind, stale = "f16 conversion", copy.deepcopy(model)
                stale.vol = before.vol
            elif name in STATE_OF:
                attr = STATE_OF[name]
                old = baked_from.get(name)
                if old is not None and repr(old) != repr(getattr(model, attr)):
                    kind, stale = "rebake", copy.deepcopy(model)
                    setattr(stale, attr, old)
                baked_from[name] = copy.deepcopy(getattr(model, attr))
            elif name in TABLE_OPS:
                kind, stale = "table, light or projection", copy.deepcopy(model)
                stale.tf, stale.tf2 = before.tf, before.tf2
                stale.light, stale.proj = before.light, before.proj
                if _equal((stale.tf, stale.tf2, stale.light, stale.proj),
                          (model.tf, model.tf2, model.light, model.proj)):
                    kind = None   # (an off that was off already)
            if kind is None or probe is None:
                continue
            recipe, old_recipe = model.expect(probe), stale.expect(probe)
            seen[kind] += 1
            if "status" in old_recipe:   # the stale library would have refused the frame
                continue
            new = reference(pkg, orc, arrays, model, probe, recipe)
            old = reference(pkg, orc, arrays, stale, probe, old_recipe)
            blind[kind] += _words_equal(new, old)
    print("blind probes: " + ", ".join(f"{k} {blind[k]}/{seen[k]}" for k in seen)
          + f"; all {sum(blind.values())}/{sum(seen.values())}")
    for kind in ("new contents", "f16 conversion", "rebake", "table, light or projection"):
        assert seen[kind] >= 8 and 8 * blind[kind] <= seen[kind], (kind, blind[kind], seen[kind])
    assert 8 * sum(blind.values()) <= sum(seen.values())


# ---- API completeness ----

# the C functions an op calls (api.py), the getters of the census, the calls of the probes
OP_API = {
    "init_distribution": ("vr_init_distribution", "vr_init_distribution_f16"),
    "convert_f16": ("vr_convert_f16",), "init_codec": ("vr_init_codec",),
    "freeCudaBuffers": ("freeCudaBuffers",), "init_gmm": ("vr_init_gmm", "vr_init_gmm_f16"),
    "free_gmm": ("vr_free_gmm",), "gmm_select": ("vr_gmm_select",),
    "convert_gmm_f16": ("vr_convert_gmm_f16",), "bake_stats": ("vr_bake_stats",),
    "release_stats": ("vr_release_stats",), "bake_weighted": ("vr_bake_weighted",),
    "release_weighted": ("vr_release_weighted",), "bake_quantile": ("vr_bake_quantile",),
    "release_quantile": ("vr_release_quantile",), "bake_distance": ("vr_bake_distance",),
    "release_distance": ("vr_release_distance",), "bake_crossing": ("vr_bake_crossing",),
    "release_crossing": ("vr_release_crossing",), "bake_gradient": ("vr_bake_gradient",),
    "release_gradient": ("vr_release_gradient",), "bake_gmm_stats": ("vr_bake_gmm_stats",),
    "release_gmm_stats": ("vr_release_gmm_stats",), "bake_gmm_range": ("vr_bake_gmm_range",),
    "release_gmm_range": ("vr_release_gmm_range",), "bake_gmm_quantile": ("vr_bake_gmm_quantile",),
    "release_gmm_quantile": ("vr_release_gmm_quantile",), "set_bin_weights": ("vr_set_bin_weights",),
    "clear_bin_weights": (), "set_query_range": ("vr_set_query_range",),
    "set_quantile": ("vr_set_quantile",), "set_quantile_spread": ("vr_set_quantile_spread",),
    "clear_quantile": ("vr_clear_quantile",), "set_query_target": ("vr_set_query_target",),
    "clear_query_target": (), "set_query_target_region": ("vr_set_query_target_region",),
    "set_isovalue": ("vr_set_isovalue",), "set_crossing_weights": ("vr_set_crossing_weights",),
    "clear_crossing_weights": (), "set_gmm_range": ("vr_set_gmm_range",),
    "clear_gmm_range": ("vr_clear_gmm_range",),
    "set_transfer_function": ("vr_set_transfer_function",),
    "set_transfer_function_2d": ("vr_set_transfer_function_2d",),
    "set_projection": ("vr_set_projection",), "set_light": ("vr_set_light",),
    "set_stream": ("vr_set_stream",), "set_layout_budget": ("vr_set_layout_budget",),
    "set_tuning": ("vr_set_tuning",),
}
CENSUS_API = ("vr_weighted_info", "vr_quantile_info", "vr_distance_info", "vr_crossing_info",
              "vr_gradient_info", "vr_stats_info", "vr_gmm_stats_info", "vr_gmm_range_info",
              "vr_gmm_quantile_info", "vr_bin_weights", "vr_quantile", "vr_query_target",
              "vr_crossing_weights", "vr_gmm_range", "vr_transfer_function",
              "vr_transfer_function_2d", "vr_projection", "vr_light_state", "vr_volume_dtype",
              "vr_gmm_dtype", "vr_layout_info")
PROBE_API = ("vr_render", "vr_render_gmm", "vr_render_gmm_baked", "vr_plane_range",
             "vr_plane_histogram", "vr_last_kernel", "vr_last_error", "vr_last_status",
             "vr_clear_error", "vr_volume_info", "vr_codec_info", "vr_gmm_phi_table",
             "vr_gmm_quantile_steps", "vr_clear_tuning")
NOT_SWEPT = {
    "render_kernel": "the reference's entry point over vr_render: tests/test_gpu_parity.py",
    "copyInvViewMatrix": "render_kernel's camera: tests/test_gpu_parity.py",
    "initCuda": "the reference's upload over vr_init_*: the initCuda tests of test_gpu_parity.py",
    "setTextureFilterMode": "a stored flag with no effect on any supported method",
    "basicDataProcessing": "vr_bake_stats without a status",
    "dataProcessing": "flexible blocks: vr_flex_process(6)",
    "vr_synthesize": "on-device generator; the sessions upload the oracle's arrays",
    "vr_synthesize_codec": "on-device generator",
    "vr_synthesize_gmm": "on-device generator",
    "vr_synthesize_gmm_f16": "on-device generator",
    "vr_init_flex": "flexible-block tables: state apart from every plane, tests/test_gpu_parity.py",
    "vr_flex_process": "flexible blocks", "vr_flex_info": "flexible blocks",
    "vr_volume_layout": "the pitches of the records, which VR_PAD alone changes",
    "vr_count_footprint": "a count, no state: tests/test_gpu_parity.py",
    "vr_footprint_bytes": "a count, no state",
    "vr_gmm_count_footprint": "a count, no state: tests/test_gpu_gmm.py",
    "vr_gmm_count_footprint_slab": "a count, no state",
    "vr_gmm_info": "pointers of the resident slices; gmm_dtype stands for the slot in the census",
    "vr_unscatter_tiles": "assembles tile lists, no state: the tile sweeps",
    "vr_tiles_x": "pure", "vr_tiles_y": "pure", "vr_version": "pure",
    "vr_debug_wave_clock": "debug hook", "vr_debug_box_check": "debug hook",
    "vr_selftest_logf": "device self-test, no state",
    "vr_stream_read": "a measurement, no state",
    "vr_plane_kernel_ms": "a measurement of the last plane_range / plane_histogram",
    "vr_parse_codebook": "file parser, no device", "vr_parse_templates": "file parser, no device",
    "vr_parse_span_list": "file parser, no device",
    "vr_parse_fractal_histogram": "file parser, no device",
    "vr_parse_simple_histogram": "file parser, no device",
    "vr_load_reference_files": "vr_init_distribution / vr_init_codec from files: tests/test_io.py",
    "vr_load_flex_files": "vr_init_flex from files",
}


def exported_functions():
    text = open(os.path.join(ROOT, "include", "vr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    return re.findall(r"^[A-Za-z_][\w \t\*]*?\b(\w+)\s*\(", text, flags=re.M)


def test_every_exported_function_has_a_decision():
    names = exported_functions()
    assert len(names) == len(set(names)) and len(names) > 100, len(names)
    assert {"render_kernel", "vr_render", "vr_set_light", "vr_gradient_info",
            "vr_plane_histogram"} <= set(names)
    assert set(OP_API) == set(sc.OPS)
    swept = [f for fs in OP_API.values() for f in fs] + list(CENSUS_API) + list(PROBE_API)
    decided = swept + list(NOT_SWEPT)
    assert len(decided) == len(set(decided)), [f for f in decided if decided.count(f) > 1]
    assert set(decided) - set(names) == set(), set(decided) - set(names)
    assert set(names) - set(decided) == set(), \
        f"exported and neither swept nor in NOT_SWEPT: {sorted(set(names) - set(decided))}"
    assert all(isinstance(r, str) and r and "\n" not in r for r in NOT_SWEPT.values())


# ---- the host-state half against the real library ----

def clean_host_state(pkg):
    pkg.set_light(None)
    pkg.set_projection(None)
    pkg.set_transfer_function(None)
    pkg.set_transfer_function_2d(None)
    pkg.set_crossing_weights(None)
    pkg.set_query_target(None)
    pkg.set_quantile(None)
    pkg.set_bin_weights(None)
    pkg.clear_gmm_range()


def test_host_state_against_the_library(pkg, sessions):
    """the setters the header calls "host state only ... work without a GPU", and their
    bad-argument forms, of every session: applied to libvr.so and to the model, the value
    getters compared after each.  Ops that need a device are skipped."""
    applied = refused = 0
    try:
        for s in sessions:
            clean_host_state(pkg)
            model = sc.Model()
            for op in steps(s):
                if op["op"] not in HOST_OPS:
                    continue
                status = model.apply(op)
                # (a weight or target count is held against the volume only at a bake)
                apply_and_check(pkg, dict(op, status=status), None)
                applied += 1
                refused += status != sc.OK
                want = {k: v for k, v in model.census().items() if k in VALUE_KEYS}
                diff = census_differences(library_census(pkg, host_only=True), want)
                assert not diff, (s["seed"], op, diff)
    finally:
        clean_host_state(pkg)
    print(f"host state: {applied} setter calls of 48 sessions, {refused} of them refused")
    assert applied >= 300 and refused >= 20, (applied, refused)
