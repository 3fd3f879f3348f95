"""Seeded random session sweep: the library's state held to a host model across the
transitions of a long-lived process.

The other sweeps (test_gpu_random.py, _queries, _transfer, _projection, _shading, _planes)
pin every march bit for bit, each from a library that was reset and built up for that one
frame.  What is correct across transitions -- which call drops which baked plane, layout
copy or device table, what survives a new volume -- stands in include/vr.h as prose.  This
sweep holds the library to those sentences, as frames.

Every case is session_cases.session(seed): a flavour (records, records+codec, gmm, mixed),
the first volumes and 16-20 ops of the public state-changing API -- uploads of new contents
of the same shape and of other shapes, owned and adopted, convert_f16, codec and GMM
volumes whole and in z-slabs, every bake and release, every setter of the caller's state,
tables, projection, light, the layout budget, a tuning knob, and about one bad call in
eleven; a table refreshed across a change of stream (session_cases' stream scene), a side
view that makes an axis-rows copy before the records are replaced (its layout scene) and
records of another shape over resident planes (its reshape scene).  The autouse fixture resets the library around the session, never
inside it.  After every op:

  1. the op is applied to the library and to session_cases.Model; a bad call must raise
     VRError with the model's status;
  2. every getter of Model.census() must match: which planes are resident (all four query
     planes, the ten gradient planes, both statistics families, the three GMM sets with
     their baked-slice counts), the values of the caller's state, the element types, and no
     layout copy resident after a call that replaces or releases the records;
  3. one frame the model says the library must serve is rendered and compared with the
     reference of the model's current state at that feature's own bar: bit for bit
     (assert_same) for methods 10-13, tables, projection, light, gradient planes and every
     frame of a plane numpy restates; test_gpu_parity.assert_parity for methods 1/2/3/7 and
     the codec's 4/5/6; test_gpu_gmm.check for the per-step GMM mean and variance; a GMM
     mean or variance plane has no bit-exact restatement, so its frames march the plane the
     device holds (tests/test_gpu_random_transfer.py's rule), which is itself held to the
     oracle's statistic of the records each slice was baked from within test_gpu_gmm.TOL;
  4. one frame the model says the library must refuse is asked for: VRError with the
     model's status, the sentinel-filled output, float and step buffers untouched, and the
     census unchanged.

One step in four, or the next one after it at which a record or codec plane is resident (134
of the 1 144 steps), also calls plane_range or plane_histogram, against ref_histogram, and
the census after it shows that the call changed no state.  The last test of the module
holds the sweep to having had layout copies resident before the calls that must drop them.
tests/test_session_model.py proves on the CPU that the sessions reach every op and every
documented cause of a drop and that the probes would see a stale plane, copy or table.

A failure message carries the seed, the step, every op up to it and last_kernel().

Seconds per session on one MI355X, references included (the CASE lines of a run with -s):
0.32 mean / 0.63 at most; the 48 sessions (1 144 steps) take 17 s.
"""
import time

import numpy as np
import pytest

import session_cases as sc
import test_gpu_gmm
from test_gpu_parity import assert_parity
from test_gpu_random_queries import assert_same, render_frame
from test_gpu_transfer2 import _gmm_plane
from test_random_cases import camera
from test_session_model import (Arrays, apply_and_check, census_differences, library_census,
                                new_model, plane_of, reference, stat_reference, steps)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
# the ops after which no layout copy may be resident (Model.layout_zero), and over the sweep
# how many of them found one resident to drop
ZEROING = ("init_distribution", "convert_f16", "freeCudaBuffers", "release_stats")
SEEN = dict(sessions=set(), layout_scenes=set(), copies_made=set(), copies_dropped=0)


@pytest.fixture(autouse=True)
def _clean(pkg, gpu):
    """no light, no projection, no table, no query state, no planes, no tuning knob, the
    default stream and layout budget and no volume of any kind, before and after the
    session"""
    def drop():
        import torch
        torch.cuda.synchronize()
        pkg.set_light(None)
        pkg.set_projection(None)
        pkg.set_transfer_function(None)
        pkg.set_transfer_function_2d(None)
        pkg.clear_tuning()
        pkg.set_stream(None)
        pkg.set_layout_budget(None)
        pkg.set_crossing_weights(None)
        pkg.set_query_target(None)
        pkg.set_quantile(None)
        pkg.set_bin_weights(None)
        pkg.release_stats()
        pkg.clear_gmm_range()
        pkg.release_gmm_stats()
        pkg.release_gmm_range()
        pkg.release_gmm_quantile()
        for slot in (1, 0):
            pkg.gmm_select(slot)
            pkg.free_gmm()
        pkg.freeCudaBuffers()
    drop()
    yield
    drop()


class Device:
    """what the ops need of the GPU: torch, the second stream, an adopted volume's tensor"""

    def __init__(self, torch):
        self.torch = torch
        self.stream = torch.cuda.Stream()
        self.adopted = None

    def on_stream(self, model):
        """torch's own work (the output buffers' fills) on the stream the library renders on"""
        return self.torch.cuda.stream(self.stream if model.stream else None)


def frame_call(pkg, probe):
    """(the entry point, its extra descriptor fields)"""
    if probe["entry"] == "render":
        return pkg.render, {}
    return getattr(pkg, probe["entry"]), dict(volume_size=(1, 1, 1))


def check_census(pkg, model, what):
    diff = census_differences(library_census(pkg), model.census())
    assert not diff, f"{what}: census: " + "; ".join(diff)


def served_probe(pkg, orc, arrays, dev, model, probe, what):
    """render the probe and compare it with the reference of the model's state"""
    torch = dev.torch
    recipe = model.expect(probe)
    assert "status" not in recipe, f"{what}: the model refuses its own probe: {recipe}"

    def device_plane(m):
        got = _gmm_plane(pkg.gmm_stats_info(), m - 1)
        want = plane_of(pkg, orc, arrays, model, "gmm", m)
        err = float(np.max(np.abs(got - want)))
        assert err <= test_gpu_gmm.TOL, f"{what}: the GMM plane of method {m} is {err} off the " \
            "oracle's statistic of the records it was baked from"
        return got

    ref = reference(pkg, orc, arrays, model, probe, recipe, device_plane)
    call, kw = frame_call(pkg, probe)
    with dev.on_stream(model):
        got = render_frame(pkg, torch, probe, camera(pkg, probe), call, **kw)
    what = f"{what}: probe {probe} by {recipe}, kernel {pkg.last_kernel()}"
    if recipe["bar"] == "same":
        assert_same(got, ref, what)
    elif recipe["bar"] == "parity":
        assert_parity(got, ref, what)
    else:
        test_gpu_gmm.check(got, dict(out=ref[0], out_f=ref[1], out_n=ref[2]), what)
    return pkg.last_kernel()


def refused_probe(pkg, dev, model, probe, what):
    """the frame must be refused with the model's status, and nothing written"""
    torch = dev.torch
    W, H, p = probe["W"], probe["H"], probe["params"]
    call, _ = frame_call(pkg, probe)
    with dev.on_stream(model):
        out = torch.full((H * W,), SENTINEL, dtype=torch.int32, device="cuda")
        out_f = torch.full((H * W * 4,), -77.25, dtype=torch.float32, device="cuda")
        n = torch.full((H * W,), -77, dtype=torch.int32, device="cuda")
        desc = pkg.make_desc(out, W, H, camera(pkg, probe), density=p["density"],
                             brightness=p["brightness"], transfer_offset=p["toff"],
                             transfer_scale=p["tscale"], query_method=probe["method"],
                             volume_size=(1, 1, 1), d_output_f=out_f, d_steps=n)
        status, message = sc.OK, "rendered"
        try:
            call(desc)
        except pkg.VRError as e:
            status, message = e.status, str(e)
    assert status == probe["status"], \
        f"{what}: refused probe {probe}: status {status} ({message})"
    pkg._lib.load().vr_clear_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((out_f == -77.25).all()) and \
        bool((n == -77).all()), f"{what}: refused probe {probe} wrote into its buffers"


def stat_call(pkg, orc, arrays, model, stat, what):
    want = stat_reference(pkg, orc, arrays, model, stat)
    what = f"{what}: {stat}"
    if stat["call"] == "plane_range":
        lo, hi, nn = pkg.plane_range(stat["u"], stat["box"])
        bits = lambda x: np.array([x], np.float32).view(np.uint32)[0]
        assert (bits(lo), bits(hi), nn) == (bits(want[0]), bits(want[1]), want[2]), \
            f"{what}: {(lo, hi, nn)} for {want}"
    else:
        got = pkg.plane_histogram(stat["u"], stat["nu"], stat["wu"], stat["v"], stat["nv"],
                                  stat["wv"], stat["box"])
        assert got.shape == want.shape and np.array_equal(got, want), \
            f"{what}: {int(np.sum(got != want))} bins differ"


@pytest.mark.parametrize("seed", range(sc.N_SESSIONS))
def test_random_session(pkg, orc, gpu, seed):
    import torch
    t0 = time.perf_counter()
    session = sc.session(seed)
    arrays, dev = Arrays(orc), Device(torch)
    model = new_model(arrays)
    ops, kernels = steps(session), set()
    try:
        for i, op in enumerate(ops):
            done = [{k: v for k, v in o.items() if k not in ("probe", "refuse", "stat")}
                    for o in ops[:i + 1]]
            what = f"seed {seed} ({session['flavour']}) step {i} of {len(ops)}, ops so far {done}"
            try:
                assert model.apply(op) == op["status"], what
                if op["op"] in ZEROING and pkg.layout_info()["resident_bytes"] > 0:
                    SEEN["copies_dropped"] += 1
                apply_and_check(pkg, op, arrays, dev)
                torch.cuda.synchronize()
                check_census(pkg, model, what)
                if op["probe"] is not None:
                    kernels.add(served_probe(pkg, orc, arrays, dev, model, op["probe"], what))
                    model.layout_zero = False   # (the frame may have made a layout copy)
                    if i == len(session["first"]) and op["op"] == "set_tuning":
                        # the layout scene: a side view of owned fp32 records of at most 8
                        # bins gets an axis-rows copy (vr.h, vr_bake_stats)
                        SEEN["layout_scenes"].add(seed)
                        if pkg.layout_info()["resident_bytes"] > 0:
                            SEEN["copies_made"].add(seed)
                if op["refuse"] is not None:
                    refused_probe(pkg, dev, model, op["refuse"], what)
                    check_census(pkg, model, what + ": after the refused probe")
                if op["stat"] is not None:
                    stat_call(pkg, orc, arrays, model, op["stat"], what)
                    check_census(pkg, model, what + ": after " + op["stat"]["call"])
            except AssertionError as e:
                raise AssertionError(f"{e}\n  last kernel {pkg.last_kernel()}\n  {what}") from None
            except pkg.VRError as e:
                if e.status == pkg._lib.VR_ERR_HIP:   # nothing more on a device that may have faulted
                    pytest.exit(f"HIP error {e}\n  last kernel {pkg.last_kernel()}\n  {what}", 3)
                raise AssertionError(f"VRError {e.status}: {e}\n  last kernel "
                                     f"{pkg.last_kernel()}\n  {what}") from None
    finally:
        torch.cuda.synchronize()
        pkg.set_stream(None)
    SEEN["sessions"].add(seed)
    print(f"\nCASE session seed {seed} {session['flavour']} steps {len(ops)} kernels "
          f"{len(kernels)} seconds {time.perf_counter() - t0:.2f}")


def test_layout_copies_were_resident_before_their_drop():
    """the census's "no layout copy after a call that replaces or releases the records" is
    worth something only if copies were there: every layout scene of the sweep (six records
    sessions start with one) made its axis-rows copy, and each of those sessions goes on to
    an op that must drop it.  Holds after a run of all 48 sessions; a partial run proves
    nothing either way."""
    if len(SEEN["sessions"]) < sc.N_SESSIONS:
        return
    print(f"layout scenes {sorted(SEEN['layout_scenes'])}, copies made in "
          f"{sorted(SEEN['copies_made'])}, zeroing ops that found a copy {SEEN['copies_dropped']}")
    assert len(SEEN["layout_scenes"]) >= 6, SEEN
    assert SEEN["copies_made"] == SEEN["layout_scenes"], SEEN
    assert SEEN["copies_dropped"] >= len(SEEN["layout_scenes"]), SEEN
