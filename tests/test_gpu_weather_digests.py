"""The weather kernels (csrc/weather.hip) held bit for bit to the bytes recorded before their store epilogues, table
fills and launch plans were put on shared pieces.  The parity paths have the CPU oracle (tests/test_gpu_kernels.py); the Philox
paths — throughput-mode fog through the strip and the tile kernel, Philox night, awseg_weather_batch — have no bit-exact
reference, so tests/golden/weather_digests.json holds, per case, the sha256 of the raw output bytes (uint8 `out`, float32
`norm_out`, float64 `depth_out` where produced) and one plain sum per output that says which of them moved;
tests/golden/make_weather_digests.py records it from the cases built here.

Every output is a per-pixel store and the coverage map is built with atomicOr, so the bytes depend neither on the launch order
nor on the height of a fog strip (one case is recorded under two values of AWSEG_FOG_STRIP_ROWS and must give one digest).

Seams: fog strips that end inside the image and a second wave in x (70 x 256), the narrowest strip width (37 x 16), W % 4 != 0
and an output one byte off alignment (the tile kernel and its scalar stores), hw % 4 != 0 (night's scalar path), rain / snow
strips FAST and not, several y-blocks with a ragged last strip and a partly filled second x-block (200 x 392: there the 7 x 7
tile kernel has interior tiles on its aligned staging path), and the one-launch batch with every kind."""
import hashlib
import json
import os
from contextlib import contextmanager
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "weather_digests.json"
STREAK_SHAPES = ((40, 72), (33, 70), (200, 392))                    # strip FAST; strip not FAST; several blocks in y and x
STRIP_ROWS_CASE, STRIP_ROWS = "fog-philox-70x256-out+norm+depth", (7, 32)


# ----------------------------------------------------------------------------- host-made inputs (numpy generators, fixed seeds)
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _frames(b, h, w):
    return _rng(1, b, h, w).integers(0, 256, (b, h, w, 3), dtype=np.uint8)


def _dev(a, off=0):
    """`a` on the device, contiguous, its first element `off` elements behind a 16-byte aligned base."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.zeros(t.numel() + off + 16, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + t.numel()].copy_(t.reshape(-1))
    return buf[off:off + t.numel()].view(t.shape)


def _outs(b, h, w, which, off=0):
    """The requested outputs, pre-filled so that a pixel no kernel stores is seen: out (uint8), norm (float32), depth (float64)."""
    o = {}
    if "out" in which:
        o["out"] = _dev(np.full((b, h, w, 3), 7, np.uint8), off)
    if "norm" in which:
        o["norm"] = _dev(np.full((b, 3, h, w), -5.0, np.float32))
    if "depth" in which:
        o["depth"] = _dev(np.full((b, h, w), -1.0, np.float64))
    return o


@contextmanager
def _strip_rows(rows):
    """AWSEG_FOG_STRIP_ROWS for the calls inside (the launcher reads it per call); None leaves the launcher's own choice."""
    old = os.environ.pop("AWSEG_FOG_STRIP_ROWS", None)
    if rows is not None:
        os.environ["AWSEG_FOG_STRIP_ROWS"] = str(rows)
    try:
        yield
    finally:
        os.environ.pop("AWSEG_FOG_STRIP_ROWS", None)
        if old is not None:
            os.environ["AWSEG_FOG_STRIP_ROWS"] = old


def _drops(h, w, seed):
    """Two frames of rain at intensities 0.2 / 0.8 (thin and thick drops), two of snow; (intensity, primitives) per frame."""
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data import preprocessing as P
    rs = np.random.RandomState(seed + 131 * h + w)
    rain = [P.draw_rain(h, w, v, rs) for v in (0.2, 0.8)]
    snow = [P.draw_snow(h, w, v, rs)[:2] for v in (0.2, 0.8)]
    assert all({1, 3} <= set(d[1][:, 4].tolist()) for d in rain) and all({2, 8} <= set(d[1][:, 2].tolist()) for d in snow)
    return rain, snow


# ----------------------------------------------------------------------------- one runner per entry point -> {name: tensor}
def run_fog(ops, h, w, which, mode, rows=None, off=0):
    """mode: "philox" (strip or tile kernel, as the launcher decides), "noise" (parity), "depth" (ops.fog(depth=...))."""
    b = 2
    imgs, o = _dev(_frames(b, h, w)), _outs(b, h, w, which, off)
    jobs = ops.fog_jobs([0, 1], [0.5, 0.3], seeds=[0x1234567 + h, (7 << 40) + w])
    kw = dict(out=o.get("out"), norm_out=o.get("norm"))
    with _strip_rows(rows):
        if mode == "philox":
            ops.fog(imgs, jobs, depth_out=o.get("depth"), **kw)
        elif mode == "noise":
            ops.fog(imgs, jobs, noise=_dev(_rng(2, h, w).standard_normal((b, h, w)) * 10.0), **kw)
        else:
            ops.fog(imgs, jobs, depth=_dev(_rng(3, h, w).uniform(1.0, 100.0, (b, h, w))), **kw)
    return o


def run_synthetic_depth(ops, h, w, with_noise):
    jobs = ops.fog_jobs([0, 1], [0.5, 0.3], seeds=[11, 12])
    noise = _dev(_rng(4, h, w).standard_normal((2, h, w)) * 10.0) if with_noise else None
    return {"depth": ops.synthetic_depth(h, w, jobs, "cuda", noise=noise)}


def run_night(ops, h, w, philox):
    b = 2
    imgs, o = _dev(_frames(b, h, w)), _outs(b, h, w, ("out", "norm"))
    jobs = ops.night_jobs([0, 1], [0.8, 0.55], [0.6, 0.4], seeds=[21 + h, 22 + w])
    noise = None if philox else _dev(_rng(5, h, w).normal(0.0, 5.0 / 255.0, (b, h, w, 3)))
    ops.night(imgs, jobs, noise=noise, out=o["out"], norm_out=o["norm"])
    return o


def run_streak(ops, h, w, kind):
    """kind: "rain", "snow3", "snow7"."""
    b = 2
    imgs, o = _dev(_frames(b, h, w)), _outs(b, h, w, ("out", "norm"))
    rain, snow = _drops(h, w, 6)
    if kind == "rain":
        jobs, prims = ops.prim_jobs([0, 1], [d[0] for d in rain], [d[1] for d in rain])
        ops.rain(imgs, jobs, prims, out=o["out"], norm_out=o["norm"])
    else:
        jobs, prims = ops.prim_jobs([0, 1], [d[0] for d in snow], [d[1] for d in snow], [int(kind[-1])] * b)
        ops.snow(imgs, jobs, prims, out=o["out"], norm_out=o["norm"])
    return o


def run_batch(ops, b, h, w):
    """Every kind in one launch: b = 5 one frame each; b = 8 two rain and two snow frames (and two fog frames)."""
    N = ops.N
    kinds = {5: [N.WEATHER_RAIN, N.WEATHER_CLEAN, N.WEATHER_FOG, N.WEATHER_NIGHT, N.WEATHER_SNOW],
             8: [N.WEATHER_SNOW, N.WEATHER_FOG, N.WEATHER_RAIN, N.WEATHER_CLEAN, N.WEATHER_NIGHT, N.WEATHER_RAIN, N.WEATHER_FOG, N.WEATHER_SNOW]}[b]
    imgs, o = _dev(_frames(b, h, w)), _outs(b, h, w, ("out", "norm"))
    rain, snow = _drops(h, w, 7)
    wj = np.zeros(b, dtype=N.WEATHER_JOB)
    lists, offs, seen = {N.WEATHER_RAIN: [], N.WEATHER_SNOW: []}, {N.WEATHER_RAIN: 0, N.WEATHER_SNOW: 0}, {N.WEATHER_RAIN: 0, N.WEATHER_SNOW: 0}
    for i, k in enumerate(kinds):
        wj[i]["kind"], wj[i]["image"] = k, i
        if k == N.WEATHER_FOG:
            fj = ops.fog_jobs([i], [0.3 + 0.05 * i], [100 + i])[0]
            wj[i]["a"], wj[i]["b"], wj[i]["seed"] = fj["beta"], fj["atmos"], fj["seed"]
        elif k == N.WEATHER_NIGHT:
            wj[i]["a"], wj[i]["b"], wj[i]["seed"] = 0.8, 0.6, 200 + i
        elif k in lists:
            inten, pl = (rain if k == N.WEATHER_RAIN else snow)[seen[k]]
            seen[k] += 1
            wj[i]["a"], wj[i]["prim_offset"], wj[i]["prim_count"] = float(inten), offs[k], len(pl)
            lists[k].append(pl)
            offs[k] += len(pl)
    rd = np.concatenate(lists[N.WEATHER_RAIN] + [np.zeros((1, 5), np.int32)])
    sf = np.concatenate(lists[N.WEATHER_SNOW] + [np.zeros((1, 3), np.int32)])
    assert ops.weather_batch(imgs, wj, rd, sf, o["norm"], out=o["out"])
    return o


def run_normalize(ops, h, w, with_sel):
    b = 3
    imgs, norm = _dev(_frames(b, h, w)), _outs(b, h, w, ("norm",))["norm"]
    sel = torch.tensor([2, 0], dtype=torch.int32, device="cuda") if with_sel else None
    ops.normalize(imgs, out=norm, sel=sel)
    return {"norm": norm}


def run_lut3(ops, h, w):
    b = 3
    luts = _dev(_rng(8).integers(0, 256, (2, 3, 256), dtype=np.uint8))
    out = _outs(b, h, w, ("out",))["out"]
    ops.lut3_apply(_dev(_frames(b, h, w)), luts, torch.tensor([1, -1, 0], dtype=torch.int32, device="cuda"), out=out)
    return {"out": out}


# ----------------------------------------------------------------------------- the cases
def cases():
    """{case id: callable(ops) -> {name: tensor}}, in a fixed order."""
    out = {}
    every = ("out", "norm", "depth")
    for h, w in ((70, 256), (37, 16)):                               # Philox fog, strip kernel
        for which in (("out",), ("norm",), every):
            out[f"fog-philox-{h}x{w}-{'+'.join(which)}"] = lambda ops, h=h, w=w, which=which: run_fog(ops, h, w, which, "philox")
    for rows in STRIP_ROWS:
        out[f"{STRIP_ROWS_CASE}-rows{rows}"] = lambda ops, rows=rows: run_fog(ops, 70, 256, every, "philox", rows=rows)
    for which in (("out",), ("norm",), every):                       # Philox fog, tile kernel: W % 4 != 0
        out[f"fog-philox-33x70-{'+'.join(which)}"] = lambda ops, which=which: run_fog(ops, 33, 70, which, "philox")
    out["fog-philox-40x72-out+norm+depth-out_off1"] = lambda ops: run_fog(ops, 40, 72, every, "philox", off=1)
    for h, w in ((40, 72), (33, 70)):
        out[f"fog-noise-{h}x{w}"] = lambda ops, h=h, w=w: run_fog(ops, h, w, ("out", "norm"), "noise")
        out[f"fog-depth-{h}x{w}"] = lambda ops, h=h, w=w: run_fog(ops, h, w, ("out", "norm"), "depth")
    for with_noise in (False, True):
        out[f"synthetic_depth-33x70-{'noise' if with_noise else 'philox'}"] = lambda ops, n=with_noise: run_synthetic_depth(ops, 33, 70, n)
    for h, w in ((40, 72), (33, 35)):                                # vector path; hw % 4 != 0
        for philox in (True, False):
            out[f"night-{'philox' if philox else 'noise'}-{h}x{w}"] = lambda ops, h=h, w=w, p=philox: run_night(ops, h, w, p)
    for kind in ("rain", "snow3", "snow7"):
        for h, w in STREAK_SHAPES:
            out[f"{kind}-{h}x{w}"] = lambda ops, h=h, w=w, kind=kind: run_streak(ops, h, w, kind)
    out["batch-5x40x72"] = lambda ops: run_batch(ops, 5, 40, 72)
    out["batch-8x64x128"] = lambda ops: run_batch(ops, 8, 64, 128)
    for h, w in ((40, 72), (33, 35)):
        for with_sel in (False, True):
            out[f"normalize-{h}x{w}{'-sel' if with_sel else ''}"] = lambda ops, h=h, w=w, s=with_sel: run_normalize(ops, h, w, s)
    out["lut3-40x72"] = lambda ops: run_lut3(ops, 40, 72)
    return out


def digest(outputs):
    """{"sha256": of the outputs' raw bytes in name order, "sums": per output, the sum of its bytes (uint8) or 32-bit words}."""
    h, sums = hashlib.sha256(), {}
    for name in sorted(outputs):
        a = np.ascontiguousarray(outputs[name].detach().cpu().numpy())
        h.update(name.encode() + b":" + a.tobytes())
        sums[name] = int(a.reshape(-1).view(np.uint8 if a.dtype == np.uint8 else np.uint32).astype(np.uint64).sum())
    return {"sha256": h.hexdigest(), "sums": sums}


def record(ops):
    """{case id: digest}: what the recorder writes and the tests compare with."""
    return {name: digest(fn(ops)) for name, fn in cases().items()}


# ----------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def ops(native):
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    return ops


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


CASES = cases()


def test_the_recorded_cases_are_the_cases_built_here(golden):
    assert sorted(golden) == sorted(CASES)


def test_the_misaligned_output_really_starts_off_alignment():
    assert _outs(1, 4, 4, ("out",), off=1)["out"].data_ptr() % 4 == 1 and _outs(1, 4, 4, ("out",))["out"].data_ptr() % 16 == 0


def test_fog_strip_bytes_do_not_depend_on_the_strip_height(golden):
    """The same frames under AWSEG_FOG_STRIP_ROWS = 7, 32 and the launcher's own choice: one digest."""
    got = {golden[f"{STRIP_ROWS_CASE}-rows{rows}"]["sha256"] for rows in STRIP_ROWS} | {golden[STRIP_ROWS_CASE]["sha256"]}
    assert len(got) == 1


@pytest.mark.parametrize("name", list(CASES))
def test_weather_bytes_are_the_recorded_ones(ops, golden, name):
    got, want = digest(CASES[name](ops)), golden[name]
    assert got["sums"] == want["sums"]                               # first: says which output moved
    assert got["sha256"] == want["sha256"]
