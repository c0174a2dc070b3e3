"""-m gpu: awseg_dehaze_guided against the numpy float32 model of tests/guided_ref.py, bit for bit (restored frames, airlight,
transmission, both counter tensors: the header states every operation and the order of the box sums' additions, so there is no
tolerance); its launches replayed inside the fenced arena of tests/fenced.py with the prototypes of include/awseg_restore.h; and the
harness under refine: guided and with the fidelity counters of the restored frames, end to end."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import fenced
from tests import guided_ref as G
from tests import quality_ref as Q
from tests import restore_ref as R

pytestmark = pytest.mark.gpu
RESTORE_HEADER = Path(__file__).resolve().parents[1] / "include" / "awseg_restore.h"
TH, TW = 32, 64                                       # AWSEG_DEHAZE_TILE_H, AWSEG_DEHAZE_TILE_W: the tiles of the guided kernels too


@pytest.fixture(scope="module")
def P(native):
    from types import SimpleNamespace
    import adverse_weather_semantic_segmentation_robustness_benchmark_amd as pkg
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import loader
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation import harness, metrics
    return SimpleNamespace(pkg=pkg, ops=ops, N=native, loader=loader, harness=harness, metrics=metrics, RobustnessMetrics=pkg.RobustnessMetrics)


# --------------------------------------------------------------------------------------------------------------------- frames
def rendered(seed, b, h, w):
    return Q.rendered_frames(seed, b, 3, h, w)[0]


def random(seed, b, h, w):
    return Q.random_frames(seed, b, 3, h, w)[0]


def constant(seed, b, h, w):
    return np.broadcast_to(R.normalise(np.full((3, 1, 1), 0.625, np.float32)), (b, 3, h, w)).copy()


def dark(seed, b, h, w):
    """Nothing brighter than 0.06: the airlight estimate is below airlight_min in every channel and the floor engages."""
    return R.normalise(0.06 * np.random.default_rng(seed).random((b, 3, h, w)))


def nonfinite(seed, b, h, w):
    x = random(seed, b, h, w)
    flat = x.reshape(-1)
    idx = np.random.default_rng(seed + 1).choice(flat.size, size=min(9, flat.size // 4), replace=False)
    flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), idx.size)
    return x


SMALL, BELOW, TILE, ABOVE = (2, 3, 5, 7), (1, 3, TH - 1, TW - 1), (1, 3, TH, TW), (1, 3, TH + 1, TW + 1)
ODD, WIDE = (3, 3, 31, 53), (2, 3, TH + 11, 2 * TW + 12)
# (id, shape, radius, guided radius, frames, float32 elements past a 16-byte boundary, transmission asked for)
CASES = [("smaller than every window", SMALL, 7, 28, random, 0, True), ("one short of a tile", BELOW, 7, 28, random, 0, False),
         ("one tile", TILE, 7, 28, rendered, 0, True), ("one past a tile", ABOVE, 7, 28, random, 0, True),
         ("scalar path, distinct frames", ODD, 7, 28, rendered, 0, True), ("16-byte path, 2 x 3 tiles", WIDE, 7, 28, rendered, 0, True),
         ("16-byte path, no transmission", WIDE, 7, 28, rendered, 0, False),
         ("W % 4 == 0, 4 bytes off alignment", WIDE, 7, 28, rendered, 1, True)]
CASES += [(f"{name} r={r} R={gr}", shape, r, gr, frames, 0, gr != 8) for name, shape, frames in (("odd", ODD, random), ("wide", WIDE, rendered))
          for r, gr in ((1, 1), (3, 8), (7, 32), (15, 32))]
CASES += [("constant frame", ABOVE, 7, 28, constant, 0, True), ("dark frame: the floor engages", ABOVE, 7, 28, dark, 0, True),
          ("NaN, +inf and -inf pixels", ABOVE, 7, 28, nonfinite, 0, True), ("NaN, +inf and -inf pixels, 16-byte path", TILE, 3, 9, nonfinite, 0, True)]


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


def differing(got: torch.Tensor, want: np.ndarray) -> str:
    diff = np.nonzero(got.cpu().numpy().view(np.int32) != want.view(np.int32))
    return "" if diff[0].size == 0 else f"{diff[0].size} of {want.size} values differ, first at {[int(d[0]) for d in diff]}"


def test_constants_mirror_the_header(P):
    import re
    defines = dict(re.findall(r"#define\s+(AWSEG_\w+)\s+(\d+)", RESTORE_HEADER.read_text()))
    assert (int(defines["AWSEG_DEHAZE_TILE_H"]), int(defines["AWSEG_DEHAZE_TILE_W"])) == (TH, TW)
    assert P.ops.GUIDED_ROW == int(defines["AWSEG_GUIDED_ROW"]) == G.ROW and P.ops.GUIDED_MAX_RADIUS == int(defines["AWSEG_GUIDED_MAX_RADIUS"])


@pytest.mark.parametrize("name,shape,radius,guided_radius,frames,shift,ask", CASES, ids=[c[0] for c in CASES])
def test_dehaze_guided_equals_the_numpy_model_bit_for_bit(P, name, shape, radius, guided_radius, frames, shift, ask):
    b, _, h, w = shape
    x = frames(11, b, h, w)
    want, want_a, want_t, want_stats, want_guided = G.dehaze_guided(x, radius=radius, guided_radius=guided_radius)
    stats, guided = P.ops.new_dehaze_stats("cuda", 1), P.ops.new_guided_stats("cuda", 1)
    out = on_device(np.zeros_like(x), shift)
    res = P.ops.dehaze_guided(on_device(x, shift), stats, guided, radius=radius, guided_radius=guided_radius, out=out, transmission=ask)
    torch.cuda.synchronize()
    assert len(res) == (3 if ask else 2) and res[0].data_ptr() == out.data_ptr()
    got, got_a = res[:2]
    assert same_bits(got_a, want_a), (got_a.cpu().numpy(), want_a)
    if ask:
        assert not differing(res[2], want_t), "transmission: " + differing(res[2], want_t)
    assert not differing(got, want), differing(got, want)
    assert stats.cpu().numpy().tolist() == want_stats.tolist()
    assert guided.cpu().numpy().tolist() == want_guided.tolist()
    assert want_guided[0, G.PIXELS] == b * h * w
    if frames is constant:
        assert same_bits(got_a, np.full((b, 3), 0.625, np.float32)) and float((got - on_device(x)).abs().max()) < 1e-5
    if frames is dark:
        assert want_stats[0, R.FLOORED] == b and (want_a == np.float32(0.1)).all()
    if frames is nonfinite:
        assert want_stats[0, R.NONFINITE] == 9 and bool(torch.isfinite(got).all()) and bool(torch.isfinite(res[2]).all())


def test_other_parameters_and_normalisations_reach_the_kernel(P):
    x = rendered(3, 2, 21, 36)
    mean, std = np.array([0.4, 0.5, 0.45], np.float32), np.array([0.25, 0.2, 0.3], np.float32)
    seen = {}
    for eps in (1e-4, 1e-2):
        kw = {"radius": 3, "omega": 0.8, "t_min": 0.25, "airlight_min": 0.3, "guided_radius": 6, "guided_eps": eps}
        want, want_a, want_t, want_stats, want_guided = G.dehaze_guided(x, mean=mean, std=std, **kw)
        stats, guided = P.ops.new_dehaze_stats("cuda", 1), P.ops.new_guided_stats("cuda", 1)
        got, got_a, got_t = P.ops.dehaze_guided(on_device(x), stats, guided, mean=mean, std=std, transmission=True, **kw)
        assert same_bits(got, want) and same_bits(got_a, want_a) and same_bits(got_t, want_t)
        assert stats.cpu().numpy().tolist() == want_stats.tolist() and guided.cpu().numpy().tolist() == want_guided.tolist()
        seen[eps] = want
    assert seen[1e-4].tobytes() != seen[1e-2].tobytes()
    assert G.dehaze_guided(x, radius=3, guided_radius=6)[0].tobytes() != seen[1e-2].tobytes()         # another mean / std, omega, ...
    # the default guided radius is min(4 radius, 32)
    got = P.ops.dehaze_guided(on_device(x), radius=3)[0]
    assert same_bits(got, G.dehaze_guided(x, radius=3, guided_radius=12)[0])


def test_the_guided_output_differs_from_both_refinements_of_awseg_dehaze(P):
    x = rendered(13, 1, 40, 72)
    d = on_device(x)
    guided = P.ops.dehaze_guided(d)[0]
    for refine in (0, 1):
        assert not torch.equal(guided, P.ops.dehaze(d, refine=refine)[0])
    # and awseg_dehaze is what it was: its model of tests/restore_ref.py, after guided launches in the same process
    assert same_bits(P.ops.dehaze(d, refine=1)[0], R.dehaze(x, refine=1)[0])


def test_cond_routes_frames_into_slots_of_both_tensors_and_launches_add_up(P):
    b, _, h, w = ODD
    x, y = rendered(5, b, h, w), random(6, b, h, w)
    cond = np.array([1, -1, 0], np.int32)
    *_, first, first_g = G.dehaze_guided(x, cond=cond, n_slots=3)
    *_, second, second_g = G.dehaze_guided(y, cond=cond[::-1], n_slots=3)
    stats, guided = P.ops.new_dehaze_stats("cuda", 3), P.ops.new_guided_stats("cuda", 3)
    P.ops.dehaze_guided(on_device(x), stats, guided, torch.from_numpy(cond).cuda())
    assert stats.cpu().numpy().tolist() == first.tolist() and guided.cpu().numpy().tolist() == first_g.tolist()
    assert first_g[1].tolist() != first_g[2].tolist() and first_g[1, G.PIXELS] == first_g[2, G.PIXELS] == h * w
    P.ops.dehaze_guided(on_device(y), stats, guided, torch.from_numpy(cond[::-1].copy()).cuda())
    assert stats.cpu().numpy().tolist() == (first + second).tolist() and guided.cpu().numpy().tolist() == (first_g + second_g).tolist()
    lone, lone_g = P.ops.new_dehaze_stats("cuda", 2), P.ops.new_guided_stats("cuda", 2)      # a condition that is no slot: slot 0 only
    P.ops.dehaze_guided(on_device(x), lone, lone_g, torch.tensor([5, 1, -3], dtype=torch.int32, device="cuda"))
    assert lone[0].cpu().numpy().tolist() == first[0].tolist() and not lone[1].any()
    assert lone_g[0].cpu().numpy().tolist() == first_g[0].tolist() and not lone_g[1].any()


def test_frames_do_not_depend_on_their_batch_mates(P):
    x = rendered(8, 3, 40, 72)
    whole, a_whole, t_whole = P.ops.dehaze_guided(on_device(x), transmission=True)
    for b in range(3):
        one, a_one, t_one = P.ops.dehaze_guided(on_device(x[b:b + 1]), transmission=True)
        assert torch.equal(one[0], whole[b]) and torch.equal(a_one[0], a_whole[b]) and torch.equal(t_one[0], t_whole[b])


# --------------------------------------------------------------------------------------------------------------------- fences
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "4 bytes off alignment"])
def test_fenced_replay_writes_nothing_outside_its_buffers(P, monkeypatch, shift):
    """The launch of ops.dehaze_guided recorded and replayed by tests/fenced.py with the extension header's prototypes: 64 KiB of
    fence around restored, airlight, transmission, both counter tensors and a workspace of exactly awseg_dehaze_guided_workspace
    bytes; outputs and workspace poisoned with three bytes.  No fence byte changes, every output bit equals the plain run whatever
    the poison, no output element is left unwritten, the input is untouched, and a second call on the dirty workspace gives the same
    again."""
    protos = {**fenced.parse_header(), **fenced.parse_header(RESTORE_HEADER)}
    assert [p.name for p in protos["awseg_dehaze_guided"]][-2:] == ["workspace", "stream"] and protos["awseg_dehaze_guided"][0].const
    monkeypatch.setattr(fenced, "parse_header", lambda path=None: protos)         # record() asks it for the launchers' parameters
    b, _, h, w = WIDE if shift == 0 else ODD                          # 16-byte path; scalar path off alignment
    x = on_device(rendered(13, b, h, w), shift)
    cond = torch.tensor([0, 1, 0][:b], dtype=torch.int32, device="cuda")
    stats, guided = P.ops.new_dehaze_stats("cuda", 3), P.ops.new_guided_stats("cuda", 3)
    stats[1, 4], guided[2, 2] = 17, 23                                # accumulators: what they held stays
    out = on_device(np.zeros((b, 3, h, w), np.float32), shift)
    trace = fenced.Trace()
    with fenced.record(trace):
        restored, airlight, t = P.ops.dehaze_guided(x, stats, guided, cond, out=out, transmission=True)
    torch.cuda.synchronize()
    want, want_a, want_t, want_stats, want_guided = G.dehaze_guided(x.cpu().numpy(), cond=[0, 1, 0][:b], n_slots=3)
    want_stats[1, 4] += 17
    want_guided[2, 2] += 23
    assert same_bits(restored, want) and same_bits(airlight, want_a) and same_bits(t, want_t)
    assert stats.cpu().numpy().tolist() == want_stats.tolist() and guided.cpu().numpy().tolist() == want_guided.tolist()
    assert [l.name for l in trace.launches] == ["awseg_dehaze_guided"]
    sized = P.N.lib().awseg_dehaze_guided_workspace(b, h, w)
    assert sized == P.ops.dehaze_guided_workspace_bytes(b, h, w)
    assert [buf.requested for buf in trace.buffers.values() if buf.requested is not None] == [sized]

    slots = fenced.plan(trace, protos, inout=("stats", "guided_stats"))
    kinds = {"/".join(sorted(s.params)): s.kind for s in slots}
    assert kinds == {"image": "in", "cond": "in", "restored": "out", "airlight": "out", "transmission": "out", "stats": "inout",
                     "guided_stats": "inout", "workspace": "scratch"}
    assert next(s for s in slots if s.params == {"workspace"}).nbytes == sized
    replay = fenced.Replay(trace, slots, "cuda", protos=protos)
    for s in slots:
        if s.params & {"image", "restored"}:
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
NEW_KEYS = ("transmission_refinement", "transmission_clamped_fraction", "mean_transmission_refinement",
            "mean_transmission_clamped_fraction", "restoration_refine")


def _run(P, model, ds, ensemble, restoration=None, frames=None, **state):
    """eval_batch over ds -> (state, results).  `frames`: what each batch's images are replaced with."""
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    st = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, ensemble, restoration=restoration, **state)
    for batch in ds.batches(2):
        images = batch["image"]
        if frames is not None:
            images = frames(images, st.acc.cond_ids(batch["weather_condition"]))
        P.harness.eval_batch(model, st, images, batch["label"], batch["weather_condition"], metrics)
    return st, P.harness.finalize(st, metrics)


@pytest.mark.parametrize("ensemble", [True, False], ids=["ensemble", "single model"])
def test_harness_scores_the_guided_frames_and_leaves_the_opening_as_it_was(P, ensemble):
    from tests.test_gpu_paired import _dataset, _model
    from tests.test_gpu_strata import _single_model
    model = _model() if ensemble else _single_model(P)
    ds = _dataset(P, n=3, hw=(64, 128), kinds=("fog", "night"), schedule="round_robin")      # one frame per condition, batches of 2 and 1
    conditions = list(ds.weather_conditions)
    opening = P.harness.restoration_option({"evaluation.restoration": {"refine": "opening"}})
    # (the opening before any guided call of this test; other tests of the process may have made theirs: the second run below is
    # made after this test's)
    st_before, before = _run(P, model, ds, ensemble, opening)
    assert st_before.restoration_guided is None and st_before.restored_quality is None

    option = P.harness.restoration_option({"evaluation.restoration": {"refine": "guided", "guided_radius": 16, "guided_eps": 1e-2}})
    st_on, on = _run(P, model, ds, ensemble, option)
    params = {"guided_radius": 16, "guided_eps": 1e-2}
    hand, hand_g = P.ops.new_dehaze_stats("cuda", 1 + len(conditions)), P.ops.new_guided_stats("cuda", 1 + len(conditions))
    st_hand, by_hand = _run(P, model, ds, ensemble, frames=lambda x, cond: P.ops.dehaze_guided(x, hand, hand_g, cond, **params)[0])
    rs = st_on.restoration
    assert torch.equal(rs["counts"], st_hand.acc.counts) and int(rs["counts"].sum()) > 0 and int(rs["oob"].item()) == 0
    assert torch.equal(rs["stats"], hand) and torch.equal(st_on.restoration_guided["stats"], hand_g)
    assert int(hand_g[0, G.PIXELS]) == len(ds) * 64 * 128 == int(hand[0, R.PIXELS])
    assert not torch.equal(rs["counts"], st_before.restoration["counts"]) or not torch.equal(rs["stats"], st_before.restoration["stats"])
    assert repr(on["overall_miou_restored"]) == repr(by_hand["overall_miou"])
    for c in conditions:
        assert repr(on[f"miou_{c}_restored"]) == repr(by_hand[f"miou_{c}"])
    want = P.metrics.guided_metrics_from_stats(hand_g.cpu().numpy(), conditions)
    assert want and all(on[k] == v for k, v in want.items()) and on["restoration_refine"] == "guided"
    for c in conditions:
        assert 0.0 <= on[f"transmission_refinement_{c}"] <= 0.9 and 0.0 <= on[f"transmission_clamped_fraction_{c}"] <= 1.0
    assert set(on) - set(before) == set(want) | {"restoration_refine"}
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.report import report_markdown
    text = report_markdown(on)
    assert "Transmission refinement: guided filter" in text and "| Refinement | Clamped |" in text

    # the opening after the guided runs: none of the new keys, and key for key, repr for repr what it was before them
    st_after, after = _run(P, model, ds, ensemble, opening)
    assert list(after) == list(before) and all(repr(after[k]) == repr(before[k]) for k in before)
    assert not any(k.startswith(NEW_KEYS) or k.endswith("_restored") and k.startswith(("psnr", "ssim", "mse")) for k in after)
    assert torch.equal(st_after.restoration["counts"], st_before.restoration["counts"])
    assert torch.equal(st_after.restoration["stats"], st_before.restoration["stats"])


def _sweep_run(P, model, ds, ensemble, **state):
    """eval_batch over the paired batches of a sweep -> (state, results, [(images, condition names, sources, severity)])."""
    metrics = P.RobustnessMetrics(19, ds.weather_conditions)
    st = P.harness.EvalState(metrics, ds.weather_conditions, "cuda", 15, ensemble, sweep=ds.sweep, **state)
    batches = []
    for batch in ds.batches(2):
        batches.append((batch["image"].clone(), list(batch["weather_condition"]), list(batch["source"]), batch["severity"]))
        P.harness.eval_batch(model, st, batch["image"], batch["label"], batch["weather_condition"], metrics, sources=batch["source"],
                             severity=batch["severity"])
    return st, P.harness.finalize(st, metrics), batches


@pytest.mark.parametrize("refine", ["opening", "guided"])
def test_harness_measures_the_fidelity_of_the_restored_frames(P, refine):
    from tests.test_gpu_paired import _model
    from tests.test_gpu_quality import _dataset
    model = _model()
    ds = _dataset(P, n=2, hw=(64, 128))
    slots = ds.sweep.slots()
    quality = {"targets": [0.9, 0.75, 0.5]}
    option = P.harness.restoration_option({"evaluation.restoration": {"refine": refine}})
    st, on, batches = _sweep_run(P, model, ds, True, quality=quality, restoration=option)
    st_q, only_quality, _ = _sweep_run(P, model, ds, True, quality=quality)
    st_r, only_restoration, _ = _sweep_run(P, model, ds, True, restoration=option)
    fidelity = lambda res: {k for k in res if k.endswith("_restored") and not k.startswith(("miou", "overall_miou", "robustness"))  # noqa: E731
                            or k.startswith(("restoration_psnr", "restoration_ssim", "mean_restoration_psnr", "mean_restoration_ssim"))}
    assert st_q.restored_quality is None and st_r.restored_quality is None
    assert not fidelity(only_quality) and not fidelity(only_restoration) and fidelity(on)
    assert all(repr(on[k]) == repr(v) for k, v in only_quality.items()) and all(repr(on[k]) == repr(v) for k, v in only_restoration.items())
    assert set(on) == set(only_quality) | set(only_restoration) | fidelity(on)

    # by hand: dehaze every batch again, measure it against the clean frames of its sources
    clean = {s: img[i] for img, _, sources, severity in batches if severity == 0 for i, s in enumerate(sources)}
    second = P.ops.new_image_quality_stats("cuda", 1 + len(slots))
    oob = torch.zeros(1, dtype=torch.int64, device="cuda")
    for img, names, sources, severity in batches:
        cond = st.acc.cond_ids([P.loader.slot_name(n, severity) for n in names])
        restored = (P.ops.dehaze_guided(img, **st.restoration["params"]) if refine == "guided" else P.ops.dehaze(img, **st.restoration["params"]))[0]
        twins = torch.stack([clean[s] for s in sources])
        P.ops.image_quality(restored, twins, torch.arange(len(sources), dtype=torch.int32, device="cuda"), second, cond=cond, oob=oob)
    assert torch.equal(st.restored_quality["stats"], second) and int(st.restored_quality["oob"].item()) == 0 == int(oob.item())
    assert st.restored_quality["terms"] == sum(img.numel() for img, *_ in batches)
    assert second[1 + slots.index("clean")].any()                     # the clean batch against its own kept rows
    want = P.metrics.restored_quality_metrics_from_stats(second.cpu().numpy(), st.quality["stats"].cpu().numpy(), slots, ["fog", "night"], 2)
    assert {k: on[k] for k in fidelity(on)} == want
    pooled = second.cpu().numpy().copy()
    pooled[0] -= pooled[1 + slots.index("clean")]
    plain = P.metrics.quality_metrics_from_stats(pooled, slots, ["fog", "night"], 2, {})
    for n in ("fog_s1", "fog_s2", "night_s1", "night_s2", "fog", "night"):
        for stem in ("psnr", "ssim"):
            assert on[f"{stem}_{n}_restored"] == plain[f"{stem}_{n}"]
            assert on[f"restoration_{stem}_gain_{n}"] == on[f"{stem}_{n}_restored"] - on[f"{stem}_{n}"]
    assert on["mean_psnr_restored"] == plain["mean_psnr"] and "psnr_clean_restored" in on and "ssim_clean_restored" in on
    assert (on.get("restoration_refine") == "guided") == (refine == "guided")
