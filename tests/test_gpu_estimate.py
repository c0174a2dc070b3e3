"""-m gpu: awseg_weather_estimate against the numpy model of tests/estimate_ref.py, bit for bit (routes, descriptors, counter rows:
the header states every operation, so there is no tolerance); its launches replayed inside the fenced arena of tests/fenced.py with
the prototypes of include/awseg_restore.h; and the harness option `evaluation.restoration: auto` end to end."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import estimate_ref as E
from tests import fenced

pytestmark = pytest.mark.gpu
RESTORE_HEADER = Path(__file__).resolve().parents[1] / "include" / "awseg_restore.h"
CASES = E.gpu_cases()
COND = np.array([1, -1, 5], dtype=np.int32)                            # a slot, no condition, an id past the three slots


@pytest.fixture(scope="module")
def P(native):
    from types import SimpleNamespace
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics
    assert hasattr(ops, "weather_estimate")
    return SimpleNamespace(pkg=pkg, ops=ops, N=native, harness=harness, metrics=metrics, RobustnessMetrics=pkg.RobustnessMetrics)


def on_device(x: np.ndarray, shift: int = 0) -> torch.Tensor:
    """x on the device, `shift` float32 elements past a 16-byte boundary."""
    buf = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[shift:shift + x.size].view(x.shape)
    t.copy_(torch.from_numpy(x))
    assert t.data_ptr() % 16 == 4 * shift
    return t


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return got.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()


def run(P, x, shift=0, cond=None, n_slots=1, stats=None, **kw):
    stats = P.ops.new_estimate_stats("cuda", n_slots) if stats is None else stats
    route, desc = P.ops.weather_estimate(on_device(x, shift), stats, None if cond is None else torch.from_numpy(np.asarray(cond)).cuda(), **kw)
    torch.cuda.synchronize()
    return route, desc, stats


@pytest.mark.parametrize("name,x,kw,shift", CASES, ids=[c[0] for c in CASES])
def test_estimate_equals_the_numpy_model_bit_for_bit(P, name, x, kw, shift):
    want_route, want_desc, want_stats = E.estimate(x, cond=COND, n_slots=3, **kw)
    route, desc, stats = run(P, x, shift, COND, 3, **kw)
    print(name, "model", want_route.tolist(), want_stats[0].tolist(), "device", route.cpu().tolist(), stats[0].cpu().tolist())
    assert stats.cpu().numpy().tolist() == want_stats.tolist()
    assert same_bits(desc, want_desc), (desc.cpu().numpy().tolist(), want_desc.tolist())
    assert route.cpu().numpy().tolist() == want_route.tolist() and route.dtype == torch.int32
    b, _, h, w = x.shape
    assert want_stats[0, E.FRAMES] == b and want_stats[0, E.PIXELS] == b * h * w and want_stats[0, E.TO_NONE:].sum() == b
    # frame 0 in slot 2 (cond 1) alone; -1 and an id past the slots reach slot 0 only
    assert want_stats[2, E.FRAMES] == 1 and not want_stats[1].any()
    if "ragged" in name:
        assert want_stats[0, E.NONFINITE] == 3
    if "64 x 128" in name or "37 x 70" in name or "40 x 72" in name:
        assert want_stats[0, E.SEEDS] > 0 and len(set(want_route.tolist())) > 1


def test_both_load_paths_give_the_same_bits(P):
    _, x, kw, _ = CASES[4]                                              # 64 x 128: W % 4 == 0
    a = run(P, x, 0, COND, 3, **kw)
    for shift in (1, 2, 3):
        s = run(P, x, shift, COND, 3, **kw)
        assert all(torch.equal(u, v) for u, v in zip(a, s)), shift
    assert int(a[2][0, E.SEEDS]) > 0


def test_other_parameters_and_normalisations_reach_the_kernel(P):
    _, x, _, _ = CASES[2]
    mean, std = np.array([0.4, 0.5, 0.45], np.float32), np.array([0.25, 0.2, 0.3], np.float32)
    kw = {"radius": 4, "threshold": 0.11, "bright_min": 0.35, "cast_max": 0.9, "luma_max": 0.7, "dark_min": 0.2, "seed_min": 0.01}
    want = E.estimate(x, mean=mean, std=std, **kw)
    got = run(P, x, mean=mean, std=std, **kw)
    assert got[0].cpu().numpy().tolist() == want[0].tolist() and same_bits(got[1], want[1]) and got[2].cpu().numpy().tolist() == want[2].tolist()
    assert E.estimate(x, **kw)[2].tolist() != want[2].tolist()
    for other in ({"threshold": 0.5}, {"bright_min": 0.9}, {"radius": 1}):
        assert E.estimate(x, mean=mean, std=std, **{**kw, **other})[2][0, E.SEEDS] != want[2][0, E.SEEDS], other


def test_decision_seams(P):
    """A constant frame with v = 0.5 has D = 0.5 exactly: the compare with dark_min is strict, in float32.  Likewise a frame with a
    known number of seeds against seed_min."""
    half = E.constant_frame(40, 72, 0.5)
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    route, desc, _ = run(P, half, dark_min=0.5)
    assert desc.cpu().numpy()[0].tolist() == [0.5, 0.5, 0.5, 0.5, 0.5, 0.0] and route.tolist() == [E.NONE]
    assert run(P, half, dark_min=below)[0].tolist() == [E.DARK_CHANNEL]
    assert E.estimate(half, dark_min=0.5)[0].tolist() == [E.NONE] and E.estimate(half, dark_min=below)[0].tolist() == [E.DARK_CHANNEL]
    seeds = E.seeded_frame(40, 64, 10)                                  # 10 seeds in 2560 pixels: O = 1 / 256 exactly
    o = 10.0 / 2560.0
    route, desc, stats = run(P, seeds, radius=1, seed_min=o)
    assert int(stats[0, E.SEEDS]) == 10 and float(desc[0, 5]) == o and route.tolist() == [E.NONE]
    assert run(P, seeds, radius=1, seed_min=float(np.nextafter(np.float32(o), np.float32(0))))[0].tolist() == [E.TOPHAT]
    assert E.estimate(seeds, radius=1, seed_min=o)[0].tolist() == [E.NONE]


def test_two_launches_into_one_stats_tensor_add_up(P):
    _, x, kw, _ = CASES[2]
    _, y, _, _ = CASES[6]
    first = E.estimate(x, cond=COND, n_slots=3, **kw)[2]
    second = E.estimate(y, cond=COND[::-1], n_slots=3, **kw)[2]
    _, _, stats = run(P, x, 0, COND, 3, **kw)
    assert stats.cpu().numpy().tolist() == first.tolist()
    run(P, y, 0, COND[::-1].copy(), 3, stats=stats, **kw)
    assert stats.cpu().numpy().tolist() == (first + second).tolist() and int(stats[0, E.FRAMES]) == 6
    lone = run(P, x, 0, None, 2, **kw)[2]                               # no cond: slot 0 only
    assert lone[0].cpu().numpy().tolist() == first[0].tolist() and not lone[1].any()


def test_an_empty_batch_launches_nothing(P):
    stats = P.ops.new_estimate_stats("cuda", 2)
    route, desc = P.ops.weather_estimate(torch.zeros(0, 3, 8, 12, device="cuda"), stats)
    torch.cuda.synchronize()
    assert tuple(route.shape) == (0,) and tuple(desc.shape) == (0, 6) and not stats.any()
    x = on_device(E.constant_frame(8, 12, 0.5))
    keep_route, keep_desc = torch.full((1,), 7, dtype=torch.int32, device="cuda"), torch.full((1, 6), 7.0, device="cuda")
    ws = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    mean, std = E.IMAGENET_MEAN.copy(), E.IMAGENET_STD.copy()
    rc = P.N.lib().awseg_weather_estimate(P.N.ptr(x), 0, 3, 8, 12, P.N.host(mean), P.N.host(std), 7, 0.06, 0.5, 0.65, 0.5, 0.47, 0.001, None,
                                          P.N.ptr(keep_route), P.N.ptr(keep_desc), P.N.ptr(stats), 2, P.N.ptr(ws), P.N.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((keep_route == 7).all()) and bool((keep_desc == 7.0).all()) and bool((ws == 7).all()) and not stats.any()
    assert P.N.lib().awseg_weather_estimate_workspace(0) == 0 and P.N.lib().awseg_weather_estimate_workspace(5) == 320


def test_the_launcher_refuses_every_invalid_argument_with_its_code(P):
    """On device buffers: a refusal comes before any launch, so outputs, counters and workspace stay as they were."""
    b, h, w = 2, 8, 12
    x = on_device(E.constant_frame(h, w, 0.5, b))
    route, desc = torch.full((b,), 7, dtype=torch.int32, device="cuda"), torch.full((b, 6), 7.0, device="cuda")
    stats = P.ops.new_estimate_stats("cuda", 2)
    ws = torch.full((b * 64 + 16,), 7, dtype=torch.uint8, device="cuda")
    cond = torch.zeros(b, dtype=torch.int32, device="cuda")
    mean, std = E.IMAGENET_MEAN.copy(), E.IMAGENET_STD.copy()
    bad_std, bad_mean = np.array([0.2, -0.1, 0.2], np.float32), np.array([0.4, np.nan, 0.4], np.float32)
    ptr, host = P.N.ptr, P.N.host
    nan = float("nan")
    good = {"image": ptr(x), "batch": b, "channels": 3, "height": h, "width": w, "mean": host(mean), "std": host(std), "radius": 7,
            "threshold": 0.06, "bright_min": 0.5, "cast_max": 0.65, "luma_max": 0.5, "dark_min": 0.47, "seed_min": 0.001, "cond": ptr(cond),
            "route": ptr(route), "descriptors": ptr(desc), "stats": ptr(stats), "n_slots": 2, "workspace": ptr(ws), "stream": P.N.stream()}
    lib = P.N.lib()
    for name, value in [("image", None), ("mean", None), ("std", None), ("route", None), ("descriptors", None), ("stats", None),
                        ("workspace", None), ("channels", 1), ("batch", -1), ("height", 0), ("width", 0), ("n_slots", 0), ("radius", 0),
                        ("radius", 16), ("threshold", 0.0), ("threshold", 1.5), ("threshold", nan), ("bright_min", -0.5),
                        ("bright_min", 1.5), ("bright_min", nan), ("cast_max", 0.0), ("cast_max", 4.5), ("cast_max", nan),
                        ("luma_max", 0.0), ("luma_max", 1.5), ("luma_max", nan), ("dark_min", -0.5), ("dark_min", 1.0), ("dark_min", nan),
                        ("seed_min", -0.5), ("seed_min", 1.0), ("seed_min", nan), ("std", host(bad_std)), ("mean", host(bad_mean))]:
        assert lib.awseg_weather_estimate(*dict(good, **{name: value}).values()) == -1, (name, value)
    assert lib.awseg_weather_estimate(*dict(good, batch=65536).values()) == -2
    assert lib.awseg_weather_estimate(*dict(good, height=1 << 16, width=1 << 15).values()) == -2
    assert lib.awseg_weather_estimate(*dict(good, workspace=ctypes.c_void_p(ws.data_ptr() + 4)).values()) == -3
    torch.cuda.synchronize()
    assert bool((route == 7).all()) and bool((desc == 7.0).all()) and bool((ws == 7).all()) and not stats.any()
    for kw in ({"radius": 16}, {"threshold": 0}, {"seed_min": 1.0}, {"dark_min": nan}, {"route": torch.zeros(b, device="cuda")},
               {"descriptors": torch.zeros(b, 5, device="cuda")}, {"stats": torch.zeros(2, 7, dtype=torch.int64, device="cuda")}):
        with pytest.raises(ValueError):
            P.ops.weather_estimate(x, **kw)
    assert lib.awseg_weather_estimate(*good.values()) == 0 and lib.awseg_weather_estimate(*dict(good, cond=None).values()) == 0
    torch.cuda.synchronize()
    assert int(stats[0, E.FRAMES]) == 2 * b and int(stats[1, E.FRAMES]) == b and not bool((route == 7).any())


# --------------------------------------------------------------------------------------------------------------------- fences
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "4 bytes off alignment"])
def test_fenced_replay_writes_nothing_outside_its_buffers(P, monkeypatch, shift):
    """The launches of ops.weather_estimate recorded and replayed by tests/fenced.py with the prototypes of both headers: 64 KiB of
    fence around route, descriptors, the counter rows and a workspace of exactly awseg_weather_estimate_workspace bytes; outputs and
    workspace poisoned with three bytes.  No fence byte changes, every output bit equals the plain run whatever the poison, no
    output element is left unwritten, the input is untouched, and a second call on the dirty workspace gives the same again."""
    protos = {**fenced.parse_header(), **fenced.parse_header(RESTORE_HEADER)}
    assert [p.name for p in protos["awseg_weather_estimate"]][-2:] == ["workspace", "stream"] and protos["awseg_weather_estimate"][0].const
    monkeypatch.setattr(fenced, "parse_header", lambda path=None: protos)         # record() asks it for the launchers' parameters
    _, frames, kw, _ = CASES[6]                                         # 3 x 3 x 40 x 72, r = 15
    b = frames.shape[0]
    x = on_device(frames, shift)
    cond = torch.from_numpy(COND).cuda()
    stats = P.ops.new_estimate_stats("cuda", 3)
    stats[1, 1] = 17                                                  # an accumulator: what it held stays
    trace = fenced.Trace()
    with fenced.record(trace):
        route, desc = P.ops.weather_estimate(x, stats, cond, **kw)
    torch.cuda.synchronize()
    want_route, want_desc, want_stats = E.estimate(frames, cond=COND, n_slots=3, **kw)
    want_stats[1, 1] += 17
    assert route.cpu().numpy().tolist() == want_route.tolist() and same_bits(desc, want_desc)
    assert stats.cpu().numpy().tolist() == want_stats.tolist()
    assert [l.name for l in trace.launches] == ["awseg_weather_estimate"]
    sized = P.N.lib().awseg_weather_estimate_workspace(b)
    assert sized == P.ops.weather_estimate_workspace_bytes(b) == b * 64
    assert [buf.requested for buf in trace.buffers.values() if buf.requested is not None] == [sized]

    slots = fenced.plan(trace, protos, inout=("stats",))
    kinds = {"/".join(sorted(s.params)): s.kind for s in slots}
    assert kinds == {"image": "in", "cond": "in", "route": "out", "descriptors": "out", "stats": "inout", "workspace": "scratch"}
    assert next(s for s in slots if s.params == {"workspace"}).nbytes == sized
    replay = fenced.Replay(trace, slots, "cuda", protos=protos)
    for s in slots:
        if s.params & {"image"}:
            assert s.region.view.data_ptr() % 16 == 4 * shift
    after = {}
    for byte in (0x00, 0xFF, 0x7F):
        replay.run(byte)
        damage = replay.arena.check()
        assert not damage, f"poison {byte:#04x}: bytes outside a region changed: {damage}"
        for s in slots:
            if s.kind == "in":
                assert torch.equal(s.region.view, s.initial), f"input {s.region.name} was modified"
            if s.kind in ("out", "inout"):
                assert torch.equal(s.region.view, s.final), f"poison {byte:#04x}: {s.region.name} differs from the plain run"
        after[byte] = {id(s): s.region.view.clone() for s in slots if s.kind == "out"}
    for s in slots:
        if s.kind == "out":
            left = fenced.unwritten(after[0x00][id(s)], after[0xFF][id(s)], s.elem)
            assert left.numel() == 0, f"{left.numel()} elements of {s.region.name} were never written"
    replay.load()
    replay.launch()                                                    # on the workspace the last run left dirty
    assert not replay.arena.check()
    for s in slots:
        if s.kind in ("out", "inout"):
            assert torch.equal(s.region.view, s.final), s.region.name


# ----------------------------------------------------------------------------------------------------------------- end to end
CONDITIONS = ["clean", "fog", "rain", "snow", "night"]
PICKS = [("clean", None), ("fog", 0.6), ("rain", 0.5), ("snow", 0.45), ("night", 0.6)]
ROUTES = [E.NONE, E.DARK_CHANNEL, E.TOPHAT, E.TOPHAT, E.CLAHE]
AUTO = {"method": "auto", "estimator": {"seed_min": 0.05}}


@pytest.fixture(scope="module")
def tiny(P):
    """A tiny random-weight ensemble, one 128 x 256 batch from scene 0 (clean, fog 0.6, rain 0.5, snow 0.45, night 0.6) with random
    labels, and the plain run every case compares to."""
    from tests.test_gpu_paired import _model
    model = _model()
    frames, kinds = E.scene_batch(128, 256, 0, PICKS)
    assert kinds == CONDITIONS
    images = torch.from_numpy(frames).cuda()
    labels = torch.randint(0, 19, (5, 128, 256), generator=torch.Generator().manual_seed(3)).cuda()
    st_off, off = _run(P, model, images, labels)
    return model, images, labels, st_off, off


def _run(P, model, images, labels, restoration=None, frames=None):
    """eval_batch on the one batch -> (state, results).  `frames`: what the batch's images are replaced with."""
    metrics = P.RobustnessMetrics(19, CONDITIONS)
    option = None if restoration is None else P.harness.restoration_option({"evaluation.restoration": restoration})
    st = P.harness.EvalState(metrics, CONDITIONS, "cuda", 15, True, restoration=option)
    if frames is not None:
        images = frames(images, st.acc.cond_ids(CONDITIONS))
    P.harness.eval_batch(model, st, images, labels, CONDITIONS, metrics)
    return st, P.harness.finalize(st, metrics)


def _by_hand(P, images, cond, routes):
    """The frames restored by the three launchers applied by hand, frame by frame -> (restored, {method: its counters})."""
    n = 1 + len(CONDITIONS)
    stats = {"dark_channel": P.ops.new_dehaze_stats("cuda", n), "clahe": P.ops.new_relight_stats("cuda", n),
             "tophat": P.ops.new_deocclude_stats("cuda", n)}
    run = {E.DARK_CHANNEL: lambda x, c: P.ops.dehaze(x, stats["dark_channel"], c)[0],
           E.CLAHE: lambda x, c: P.ops.relight(x, stats["clahe"], c)[0],
           E.TOPHAT: lambda x, c: P.ops.deocclude(x, stats["tophat"], c)[0]}
    out = images.clone()
    for r in (E.DARK_CHANNEL, E.CLAHE, E.TOPHAT):
        members = [i for i, v in enumerate(routes) if v == r]
        if members:
            idx = torch.tensor(members, device="cuda")
            out[idx] = run[r](images[idx].contiguous(), cond[idx].contiguous())
    return out, stats


@pytest.mark.parametrize("route", ["estimated", "oracle"])
def test_harness_routes_every_frame_and_scores_it_a_second_time(P, tiny, route):
    model, images, labels, st_off, off = tiny
    st, on = _run(P, model, images, labels, {**AUTO, "route": route})
    es = st.restoration_estimate

    # the estimate: the numpy model's routes and counters, one row per condition, whatever routes the frames
    want_route, _, want_stats = E.estimate(images.cpu().numpy(), cond=np.arange(5, dtype=np.int32), n_slots=6, seed_min=0.05)
    assert want_route.tolist() == ROUTES and es["stats"].cpu().numpy().tolist() == want_stats.tolist()
    # the one host synchronisation: the routes of the one batch were read back, or, under the oracle, nothing was
    assert (es["readbacks"], es["host"] is None) == ((1, False) if route == "estimated" else (0, True))
    if route == "estimated":
        assert es["host"].is_pinned() and es["host"][:5].tolist() == ROUTES

    # off: nothing allocated, and key for key, bit for bit what the on-run reports for everything that existed before
    assert st_off.restoration is None and st_off.restoration_estimate is None and st_off.restoration_deocclude is None
    assert set(off) <= set(on) and all(repr(on[k]) == repr(off[k]) for k in off)
    assert torch.equal(st.acc.counts, st_off.acc.counts) and torch.equal(st.ece, st_off.ece)

    # the second accumulator is a plain evaluation of the frames the three launchers restore by hand
    hand = {}
    st_hand, by_hand = _run(P, model, images, labels,
                            frames=lambda x, cond: hand.setdefault("out", _by_hand(P, x, cond, ROUTES))[0])
    rs = st.restoration
    assert torch.equal(rs["counts"], st_hand.acc.counts) and int(rs["counts"].sum()) > 0 and int(rs["oob"].item()) == 0
    stats = hand["out"][1]
    assert torch.equal(rs["stats"], stats["dark_channel"]) and torch.equal(st.restoration_relight["stats"], stats["clahe"])
    assert torch.equal(st.restoration_deocclude["stats"], stats["tophat"])
    # each method saw its own frames only
    assert rs["stats"][:, 0].tolist() == [1, 0, 1, 0, 0, 0] and st.restoration_relight["stats"][:, 0].tolist() == [1, 0, 0, 0, 0, 1]
    assert st.restoration_deocclude["stats"][:, 0].tolist() == [2, 0, 0, 1, 1, 0]

    # every key of the option
    assert on["restoration_method"] == "auto" and on["restoration_route"] == route
    assert repr(on["overall_miou_restored"]) == repr(by_hand["overall_miou"])
    want = P.metrics.estimate_metrics_from_stats(want_stats, CONDITIONS, route=route)
    assert {k: on[k] for k in want} == want and on["route_accuracy"] == 1.0
    for name, s in (("relight", stats["clahe"]), ("deocclude", stats["tophat"])):
        own = getattr(P.metrics, f"{name}_metrics_from_stats")(s.cpu().numpy(), CONDITIONS)
        assert {k: on[k] for k in own if not k.startswith("restoration_")} == {k: v for k, v in own.items() if not k.startswith("restoration_")}
    for c, r in zip(CONDITIONS, ROUTES):
        assert repr(on[f"miou_{c}_restored"]) == repr(by_hand[f"miou_{c}"])
        assert on[f"restoration_gain_{c}"] == on[f"miou_{c}_restored"] - on[f"miou_{c}"]
        assert on[f"route_{E.ROUTES[r]}_fraction_{c}"] == 1.0 and on[f"route_accuracy_{c}"] == 1.0
        assert ("transmission_mean_" + c in on) == (r == E.DARK_CHANNEL) and ("relight_gain_" + c in on) == (r == E.CLAHE)
        assert ("occluder_fraction_" + c in on) == (r == E.TOPHAT)
    assert on["restoration_gain_clean"] == 0.0 and on["restoration_clean_cost"] == 0.0      # routed to none: the same frame
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    text = report_markdown({k: v if isinstance(v, str) else float(v) for k, v in on.items()})
    assert f"Method: auto, route: {route}" in text and "| Condition | none | dark_channel | clahe | tophat |" in text
    st.all_reduce()                                                    # the table-driven reduce takes the new entry's tensors


def test_a_wrong_estimate_is_applied_and_counted(P, tiny):
    """At the default seed_min the clean frame of this size goes to the top-hat: the estimated route restores it that way, the
    oracle does not, and the confusion table says so in both runs."""
    model, images, labels, _, _ = tiny
    st_e, est = _run(P, model, images, labels, "auto")
    st_o, orc = _run(P, model, images, labels, {"method": "auto", "route": "oracle"})
    assert torch.equal(st_e.restoration_estimate["stats"], st_o.restoration_estimate["stats"])
    for res in (est, orc):
        assert res["route_tophat_fraction_clean"] == 1.0 and res["route_accuracy_clean"] == 0.0 and res["route_accuracy"] == 0.8
    assert st_e.restoration_deocclude["stats"][:, 0].tolist() == [3, 1, 0, 1, 1, 0]
    assert st_o.restoration_deocclude["stats"][:, 0].tolist() == [2, 0, 0, 1, 1, 0]
    assert orc["restoration_clean_cost"] == 0.0 and "occluder_fraction_clean" in est and "occluder_fraction_clean" not in orc
    # [fog, night] alone: the estimator sees the selected frames only
    only = P.harness.restoration_option({"evaluation.restoration": AUTO, "evaluation.restoration_conditions": ["fog", "night"]})
    metrics = P.RobustnessMetrics(19, CONDITIONS)
    st = P.harness.EvalState(metrics, CONDITIONS, "cuda", 15, True, restoration=only)
    P.harness.eval_batch(model, st, images, labels, CONDITIONS, metrics)
    assert st.restoration_estimate["stats"][:, 0].tolist() == [2, 0, 1, 0, 0, 1] and st.restoration_estimate["host"][:2].tolist() == [1, 2]
    assert st.restoration["stats"][:, 0].tolist() == [1, 0, 1, 0, 0, 0] and not st.restoration_deocclude["stats"].any()


def test_the_clahe_grid_is_checked_against_the_frame(P, tiny):
    model, images, labels, _, _ = tiny
    option = P.harness.restoration_option({"evaluation.restoration": {"method": "auto", "clahe": {"grid": 16}}})
    metrics = P.RobustnessMetrics(19, CONDITIONS)
    st = P.harness.EvalState(metrics, CONDITIONS, "cuda", 15, True, restoration=option)
    with pytest.raises(ValueError, match="grid of 16 x 16"):
        P.harness.eval_batch(model, st, images[:, :, :8, :64].contiguous(), labels[:, :8, :64].contiguous(), CONDITIONS, metrics)
    assert not st.restoration_estimate["stats"].any()                  # refused as the batch comes: nothing was launched


def test_a_batch_refused_by_a_later_check_is_not_counted(P, tiny):
    """The estimate is launched behind the checks of the batch: one that eval_batch refuses leaves the estimate's counters empty."""
    model, images, labels, _, _ = tiny
    option = P.harness.restoration_option({"evaluation.restoration": AUTO})
    metrics = P.RobustnessMetrics(19, CONDITIONS)
    st = P.harness.EvalState(metrics, CONDITIONS, "cuda", 15, True, restoration=option, depth={"min": 1e-3, "target": "frame"})
    with pytest.raises(ValueError, match="depth"):                     # no depth target comes with the batch
        P.harness.eval_batch(model, st, images, labels, CONDITIONS, metrics)
    with pytest.raises(ValueError, match="depth head"):                # a target, but the model has no depth head
        P.harness.eval_batch(model, st, images, labels, CONDITIONS, metrics, depth=torch.ones(5, 128, 256, device="cuda"))
    torch.cuda.synchronize()
    assert not st.restoration_estimate["stats"].any() and st.restoration_estimate["pending"] is None


@pytest.mark.parametrize("spec", ["dark_channel", "clahe", "tophat"])
def test_the_other_methods_report_what_they_reported(P, tiny, spec):
    """Under the three single methods nothing new is allocated or launched, and the result dict is, key for key and bit for bit, the
    plain run's keys plus what the method's own launcher and host functions give by hand."""
    model, images, labels, st_off, off = tiny
    st, res = _run(P, model, images, labels, spec)
    assert st.restoration_estimate is None and not any("route_" in k or k.startswith(("estimate_", "mean_estimate_")) for k in res)
    assert (st.restoration_relight is not None, st.restoration_deocclude is not None) == (spec == "clahe", spec == "tophat")
    n = 1 + len(CONDITIONS)
    new, op, host = {"dark_channel": (P.ops.new_dehaze_stats, P.ops.dehaze, None),
                     "clahe": (P.ops.new_relight_stats, P.ops.relight, P.metrics.relight_metrics_from_stats),
                     "tophat": (P.ops.new_deocclude_stats, P.ops.deocclude, P.metrics.deocclude_metrics_from_stats)}[spec]
    hand = new("cuda", n)
    st_hand, _ = _run(P, model, images, labels, frames=lambda x, cond: op(x, hand, cond)[0])
    kw = {"degradation": P.RobustnessMetrics(19, CONDITIONS).compute_robustness_degradation_ratio}
    dehaze_rows = hand.cpu().numpy() if spec == "dark_channel" else np.zeros((n, P.ops.DEHAZE_ROW), np.int64)
    want = dict(off)
    want.update(P.metrics.restoration_metrics_from_stats(st_hand.acc.counts.cpu().numpy(), st_off.acc.counts.cpu().numpy(), dehaze_rows,
                                                         CONDITIONS, 19, **kw))
    if host is not None:
        want.update(host(hand.cpu().numpy(), CONDITIONS))
    assert set(res) == set(want) and all(repr(res[k]) == repr(want[k]) for k in want)
