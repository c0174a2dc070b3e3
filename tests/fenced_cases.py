"""The case table of tests/test_gpu_fenced.py: launcher name -> the call patterns that fence it (importing needs no GPU).

A case is one call pattern of the package's ops, written the way the family's existing GPU test calls it.  build(device) returns
(run, verify): run() makes the call on ordinary buffers and returns {name: tensor} for everything the operation defines (outputs and
in/out accumulators, pre-filled where the operation accumulates); verify(results) holds such a dict to the family's reference under
the family's EXISTING gate (`reference` / `gate` name them; no tolerance is new here).  Which argument is an input, an output or a
workspace is read from include/awseg.h when the launches are replayed (tests/fenced.py), and the workspaces are the exact-size
buffers the size functions in `sizes` returned.

    exact     two runs on ordinary buffers give identical bits (observed by the test, this column is the claim); `why` names
              the atomic that makes a row inexact
    inout     parameters whose buffers keep their contents across the call (accumulators; rows of an output the call skips)
    offsets   {parameter: bytes past a 256-byte boundary}: the launcher's documented scalar path for unaligned bases
    declines  {launcher: return code} for a shape the table asks for and the launcher documents it does not take
    partial   output parameters the operation defines only in part (named with the reason in the row)

A new launcher in include/awseg.h needs a row here (or a line in EXEMPT): tests/test_fenced.py fails until it has one.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable

import numpy as np
import torch


@dataclass(frozen=True)
class Case:
    id: str
    launchers: tuple
    build: Callable = field(repr=False, compare=False)
    reference: str = ""
    gate: str = ""
    exact: bool = True
    why: str = ""
    sizes: tuple = ()
    inout: tuple = ()
    scratch: tuple = ()
    offsets: dict = field(default_factory=dict, compare=False)
    declines: dict = field(default_factory=dict, compare=False)
    partial: tuple = ()
    shifted: tuple = ()               # parameters the row passes off 16-byte alignment (asserted by the test)
    free_workspace: bool = False      # the launcher takes a workspace of the caller's choosing (awseg_gemm_bias_act: the library's scratch)
    fence_bytes: int = 65536          # 64 KiB: more than one output row or tile of every case below


CASES: dict[str, list] = {}

# Entry points that launch nothing or are not replayable, each with its reason.
EXEMPT = {
    "awseg_abi_version": "host query",
    "awseg_header_hash": "host query",
    "awseg_error_string": "host query",
    "awseg_device_count": "host query",
    "awseg_gemm_tune": "synchronising warm-up helper that times the library's candidates on the caller's buffers; never on the hot path",
}


def add(case: Case) -> None:
    for name in case.launchers:
        CASES.setdefault(name, []).append(case)


def _ops():
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import ops
    return ops


def _oracle():
    from oracle import cpu_oracle
    cpu_oracle.build()
    return cpu_oracle


_SHIFT = 0            # elements every host-made input sits behind an aligned base (rows built through _off_alignment set it to 1)


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = (t if dtype is None else t.to(dtype)).to(device)
    if _SHIFT:
        buf = torch.empty(t.numel() + _SHIFT + 16, dtype=t.dtype, device=device)
        buf[_SHIFT:_SHIFT + t.numel()].copy_(t.reshape(-1))
        t = buf[_SHIFT:_SHIFT + t.numel()].view(t.shape)
    return t


def _off_alignment(build):
    """The same row with every input the case uploads one element behind an aligned base: the launchers that pick their vector
    path from the alignment of `logits`, `image`, `pred`, `label`, `ref_maps` take the scalar one, in the plain run and in the arena."""
    def shifted(device):
        run, verify = build(device)

        def run_shifted():
            global _SHIFT
            _SHIFT = 1
            try:
                return run()
            finally:
                _SHIFT = 0
        return run_shifted, verify
    return shifted


def _np(t):
    return t.detach().cpu().numpy()


IMAGE_SHAPES = [(9, 13), (12, 18), (16, 32)]        # hw % 4 != 0; W % 4 != 0 with hw % 4 == 0; aligned
MAP_SHAPES = [(5, 7), (6, 10), (8, 16)]             # hw % 4 != 0; hw % 4 == 0 and hw % 16 != 0; aligned


# =========================================================================================== weather, normalise, LUT, depth, density
def _images(h, w, seed):
    return np.random.RandomState(seed).randint(0, 255, (2, h, w, 3), dtype=np.uint8)


def _normalize(h, w, sel):
    def build(device):
        ops, oracle = _ops(), _oracle()
        imgs = _images(h, w, 1)

        def run():
            if not sel:
                return {"out": ops.normalize(_dev(imgs, device))}
            out = torch.full((2, 3, h, w), 7.0, device=device)
            ops.normalize(_dev(imgs, device), out=out, sel=torch.tensor([1], dtype=torch.int32, device=device))
            return {"out": out}

        def verify(r):
            got = _np(r["out"])
            assert np.array_equal(got[1], oracle.normalize(imgs[1]))
            assert np.array_equal(got[0], oracle.normalize(imgs[0])) if not sel else (got[0] == 7.0).all()
        return run, verify
    return build


for h_, w_ in IMAGE_SHAPES:
    add(Case(f"normalize-{h_}x{w_}", ("awseg_normalize",), _normalize(h_, w_, False), "oracle.cpu_oracle.normalize",
             "test_gpu_kernels.py::test_normalize_and_night_ragged_sizes (bit-exact)"))
add(Case("normalize-9x13-sel", ("awseg_normalize",), _normalize(9, 13, True), "oracle.cpu_oracle.normalize",
         "test_gpu_kernels.py::test_normalize_and_night_ragged_sizes (bit-exact)", inout=("out",)))
add(Case("normalize-9x13-out+4", ("awseg_normalize",), _normalize(9, 13, False), "oracle.cpu_oracle.normalize",
         "test_gpu_kernels.py::test_normalize_and_night_ragged_sizes (bit-exact)", offsets={"out": 4}))


def _lut(h, w, in_place):
    def build(device):
        from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.loader import style_lut
        ops, oracle = _ops(), _oracle()
        imgs = _images(h, w, 11)
        luts = np.stack([style_lut("rain"), style_lut("night")])

        def run():
            d = _dev(imgs, device)
            lut_of = torch.tensor([1, 0], dtype=torch.int32, device=device)
            return {"out": ops.lut3_apply(d, _dev(luts, device), lut_of, out=d if in_place else None)}

        def verify(r):
            got = _np(r["out"])
            assert np.array_equal(got[0], oracle.style_transfer(imgs[0], "night"))
            assert np.array_equal(got[1], oracle.style_transfer(imgs[1], "rain"))
        return run, verify
    return build


for h_, w_ in [(12, 18), (16, 32), (7, 12)]:          # H*W*3 % 4 == 0 is the launcher's condition: 9 x 13 is replaced by 7 x 12
    add(Case(f"lut3-{h_}x{w_}", ("awseg_lut3_apply",), _lut(h_, w_, False), "oracle.cpu_oracle.style_transfer",
             "test_gpu_kernels.py::test_style_transfer_lut (byte-exact)"))
add(Case("lut3-7x12-inplace", ("awseg_lut3_apply",), _lut(7, 12, True), "oracle.cpu_oracle.style_transfer",
         "test_gpu_kernels.py::test_style_transfer_lut (byte-exact)"))


def _local_contrast(h, w):
    def build(device):
        ops, oracle = _ops(), _oracle()
        imgs = _images(h, w, 21)
        depth = np.random.RandomState(2).uniform(1.0, 100.0, (h, w))

        def run():
            return {"contrast": ops.local_contrast(_dev(imgs, device))}

        def verify(r):
            for b in range(2):
                assert np.abs(_np(r["contrast"])[b] - oracle.fog_density_map(imgs[b], depth)[1]).max() <= 1e-7
        return run, verify
    return build


for h_, w_ in IMAGE_SHAPES:
    add(Case(f"local_contrast-{h_}x{w_}", ("awseg_local_contrast",), _local_contrast(h_, w_), "oracle.cpu_oracle.fog_density_map",
             "test_gpu_kernels.py::test_fog_density_map_local_contrast (1e-7 abs)"))
add(Case("local_contrast-9x13-out+4", ("awseg_local_contrast",), _local_contrast(9, 13), "oracle.cpu_oracle.fog_density_map",
         "test_gpu_kernels.py::test_fog_density_map_local_contrast (1e-7 abs)", offsets={"contrast": 4}))


def _depth_estimate(h, w, dtype):
    def build(device):
        ops, oracle = _ops(), _oracle()
        imgs = _images(h, w, 5)

        def run():                                     # ops.depth_estimate with the workspace sized by the library, not by hand
            N = ops.N
            d = _dev(imgs, device)
            out = torch.empty(2, h, w, dtype=dtype, device=device)
            ws = N.workspace.get(device, N.lib().awseg_depth_estimate_workspace(2), tag="depth")
            N.call("awseg_depth_estimate", N.ptr(d), 2, h, w, N.host(ops._TAPS), N.ptr(ws),
                   N.ptr(out if dtype == torch.float64 else None), N.ptr(out if dtype == torch.float32 else None), N.stream())
            return {"depth": out}

        def verify(r):
            for b in range(2):
                want = oracle.depth_estimate(imgs[b])
                assert np.array_equal(_np(r["depth"])[b], want if dtype == torch.float64 else want.astype(np.float32))
        return run, verify
    return build


for h_, w_ in IMAGE_SHAPES:
    for dt_ in (torch.float64, torch.float32):
        add(Case(f"depth_estimate-{h_}x{w_}-{str(dt_)[6:]}", ("awseg_depth_estimate",), _depth_estimate(h_, w_, dt_),
                 "oracle.cpu_oracle.depth_estimate", "test_gpu_kernels.py::test_depth_estimate_golden_and_ragged (bit-exact)",
                 sizes=("awseg_depth_estimate_workspace",)))


def _fog(h, w, mode, outs):
    """mode: 'two-step' (synthetic_depth + fog_apply), 'fused' (host noise), outs: subset of out / norm_out / depth_out."""
    def build(device):
        ops, oracle = _ops(), _oracle()
        imgs = _images(h, w, 5)
        noise = np.random.RandomState(6).normal(0, 10, (2, h, w))
        jobs = ops.fog_jobs([1, 0], [0.4, 0.8])

        def run():
            d = _dev(imgs, device)
            r = {}
            if "out" in outs:
                r["out"] = torch.empty_like(d)
            if "norm_out" in outs:
                r["norm_out"] = torch.empty(2, 3, h, w, device=device)
            if mode == "two-step":
                r["depth"] = ops.synthetic_depth(h, w, jobs, device, _dev(noise, device))
                ops.fog(d, jobs, depth=r["depth"], out=r.get("out"), norm_out=r.get("norm_out"))
            else:
                if "depth_out" in outs:
                    r["depth"] = torch.empty(2, h, w, dtype=torch.float64, device=device)
                ops.fog(d, jobs, noise=_dev(noise, device), out=r.get("out"), norm_out=r.get("norm_out"), depth_out=r.get("depth"))
            return r

        def verify(r):
            for j, b in enumerate((1, 0)):
                depth = oracle.synthetic_depth(noise[j])
                ref = oracle.fog(imgs[b], depth, (0.4, 0.8)[j])
                if "depth" in r:
                    assert np.array_equal(_np(r["depth"])[j], depth)
                if "out" in r:
                    assert np.array_equal(_np(r["out"])[b], ref)
                if "norm_out" in r:
                    assert np.array_equal(_np(r["norm_out"])[b], oracle.normalize(ref))
        return run, verify
    return build


_FOG_GATE = "test_gpu_kernels.py::test_weather_batched_and_fused_normalise / test_fog_night_depth_golden (bit-exact)"
for h_, w_ in IMAGE_SHAPES:
    add(Case(f"fog-two-step-{h_}x{w_}", ("awseg_synthetic_depth", "awseg_fog_apply"), _fog(h_, w_, "two-step", ("out", "norm_out")),
             "oracle.cpu_oracle.synthetic_depth / fog / normalize", _FOG_GATE))
    add(Case(f"fog-fused-{h_}x{w_}", ("awseg_fog_fused",), _fog(h_, w_, "fused", ("out", "norm_out", "depth_out")),
             "oracle.cpu_oracle.synthetic_depth / fog / normalize", _FOG_GATE))
add(Case("fog-two-step-9x13-out-only", ("awseg_fog_apply",), _fog(9, 13, "two-step", ("out",)), "oracle.cpu_oracle.fog", _FOG_GATE))
add(Case("fog-two-step-12x18-norm-only", ("awseg_fog_apply",), _fog(12, 18, "two-step", ("norm_out",)), "oracle.cpu_oracle.fog", _FOG_GATE))
add(Case("fog-fused-9x13-out-only", ("awseg_fog_fused",), _fog(9, 13, "fused", ("out",)), "oracle.cpu_oracle.fog", _FOG_GATE))
add(Case("fog-fused-12x18-norm-only", ("awseg_fog_fused",), _fog(12, 18, "fused", ("norm_out",)), "oracle.cpu_oracle.fog", _FOG_GATE))
add(Case("fog-two-step-9x13-out+1", ("awseg_fog_apply",), _fog(9, 13, "two-step", ("out", "norm_out")), "oracle.cpu_oracle.fog", _FOG_GATE,
         offsets={"out": 1, "norm_out": 4}))
add(Case("fog-fused-9x13-out+1", ("awseg_fog_fused",), _fog(9, 13, "fused", ("out", "norm_out", "depth_out")), "oracle.cpu_oracle.fog",
         _FOG_GATE, offsets={"out": 1, "norm_out": 4}))


def _night(h, w, outs):
    def build(device):
        ops, oracle = _ops(), _oracle()
        imgs = _images(h, w, 7)
        noise = np.random.RandomState(8).normal(0, 5.0 / 255.0, (2, h, w, 3))
        jobs = ops.night_jobs([1, 0], [0.7, 0.9], [0.5, 0.8])

        def run():
            d = _dev(imgs, device)
            r = {}
            if "out" in outs:
                r["out"] = torch.empty_like(d)
            if "norm_out" in outs:
                r["norm_out"] = torch.empty(2, 3, h, w, device=device)
            ops.night(d, jobs, noise=_dev(noise, device), out=r.get("out"), norm_out=r.get("norm_out"))
            return r

        def verify(r):
            for j, b in enumerate((1, 0)):
                ref = oracle.night(imgs[b], noise[j], (0.7, 0.9)[j], (0.5, 0.8)[j])
                if "out" in r:
                    assert np.array_equal(_np(r["out"])[b], ref)
                if "norm_out" in r:
                    assert np.array_equal(_np(r["norm_out"])[b], oracle.normalize(ref))
        return run, verify
    return build


_NIGHT_GATE = "test_gpu_kernels.py::test_normalize_and_night_ragged_sizes (bit-exact)"
for h_, w_ in IMAGE_SHAPES:
    add(Case(f"night-{h_}x{w_}", ("awseg_night_apply",), _night(h_, w_, ("out", "norm_out")), "oracle.cpu_oracle.night / normalize", _NIGHT_GATE))
add(Case("night-9x13-out-only", ("awseg_night_apply",), _night(9, 13, ("out",)), "oracle.cpu_oracle.night", _NIGHT_GATE))
add(Case("night-12x18-norm-only", ("awseg_night_apply",), _night(12, 18, ("norm_out",)), "oracle.cpu_oracle.night", _NIGHT_GATE))
add(Case("night-9x13-out+1", ("awseg_night_apply",), _night(9, 13, ("out", "norm_out")), "oracle.cpu_oracle.night", _NIGHT_GATE,
         offsets={"out": 1, "norm_out": 4}))


def _streak(kind, h, w, outs, ksizes=(3, 7)):
    def build(device):
        ops, oracle = _ops(), _oracle()
        imgs = _images(h, w, h * w)
        state = np.random.get_state()
        np.random.seed(3)
        if kind == "rain":
            (i0, p0), (i1, p1) = oracle.draw_rain(h, w, 0.5), oracle.draw_rain(h, w, None)
            jobs, prims = ops.prim_jobs([1, 0], [i0, i1], [p0, p1])
        else:
            (i0, p0, _), (i1, p1, _) = oracle.draw_snow(h, w, 0.5), oracle.draw_snow(h, w, None)
            jobs, prims = ops.prim_jobs([1, 0], [i0, i1], [p0, p1], ksizes)
        np.random.set_state(state)

        def run():
            d = _dev(imgs, device)
            r = {}
            if "out" in outs:
                r["out"] = torch.empty_like(d)
            if "norm_out" in outs:
                r["norm_out"] = torch.empty(2, 3, h, w, device=device)
            (ops.rain if kind == "rain" else ops.snow)(d, jobs, prims, out=r.get("out"), norm_out=r.get("norm_out"))
            return r

        def verify(r):
            for j, (b, i, p) in enumerate(((1, i0, p0), (0, i1, p1))):
                ref = oracle.rain(imgs[b], i, p) if kind == "rain" else oracle.snow(imgs[b], i, p, ksizes[j])
                if "out" in r:
                    assert np.array_equal(_np(r["out"])[b], ref)
                if "norm_out" in r:
                    assert np.array_equal(_np(r["norm_out"])[b], oracle.normalize(ref))
        return run, verify
    return build


_STREAK_GATE = "test_gpu_kernels.py::test_rain_snow_vs_oracle (bit-exact)"
for kind_ in ("rain", "snow"):
    for h_, w_ in IMAGE_SHAPES:
        add(Case(f"{kind_}-{h_}x{w_}", (f"awseg_{kind_}_apply",), _streak(kind_, h_, w_, ("out", "norm_out")),
                 f"oracle.cpu_oracle.{kind_} / normalize", _STREAK_GATE, sizes=("awseg_streak_workspace",)))
    add(Case(f"{kind_}-9x13-out-only", (f"awseg_{kind_}_apply",), _streak(kind_, 9, 13, ("out",)), f"oracle.cpu_oracle.{kind_}",
             _STREAK_GATE, sizes=("awseg_streak_workspace",)))
    add(Case(f"{kind_}-12x18-norm-only", (f"awseg_{kind_}_apply",), _streak(kind_, 12, 18, ("norm_out",)), f"oracle.cpu_oracle.{kind_}",
             _STREAK_GATE, sizes=("awseg_streak_workspace",)))
    # rain and snow want `out` dword aligned and `norm_out` 16-byte aligned (AWSEG_EALIGN otherwise): one element of each unit
    add(Case(f"{kind_}-9x13-out+4", (f"awseg_{kind_}_apply",), _streak(kind_, 9, 13, ("out", "norm_out")), f"oracle.cpu_oracle.{kind_}",
             _STREAK_GATE, sizes=("awseg_streak_workspace",), offsets={"out": 4, "norm_out": 16}))


def _density_field(h, w):
    def build(device):
        ops, oracle = _ops(), _oracle()
        u = np.random.RandomState(9).rand(2, h, w).astype(np.float32)

        def run():
            return {"density": ops.fog_density_field(["snow", "fog"], h, w, device, 0, uniform=_dev(u, device))}

        def verify(r):
            assert np.array_equal(_np(r["density"]), oracle.trainer_fog_density(["snow", "fog"], u))
        return run, verify
    return build


for h_, w_ in IMAGE_SHAPES:
    add(Case(f"density_field-{h_}x{w_}", ("awseg_fog_density_field",), _density_field(h_, w_), "oracle.cpu_oracle.trainer_fog_density",
             "test_gpu_kernels.py::test_fog_density_field_parity_mode_is_the_reference (bit-exact)"))
add(Case("density_field-9x13-out+4", ("awseg_fog_density_field",), _density_field(9, 13), "oracle.cpu_oracle.trainer_fog_density",
         "test_gpu_kernels.py::test_fog_density_field_parity_mode_is_the_reference (bit-exact)", offsets={"density": 4}))


def _density_from_depth(h, w):
    def build(device):
        ops, oracle = _ops(), _oracle()
        depth = np.random.RandomState(10).rand(2, h, w).astype(np.float32)

        def run():
            return {"density": ops.fog_density_from_depth(_dev(depth, device))}

        def verify(r):
            assert (np.abs(_np(r["density"]) - oracle.fog_density_from_depth(depth)) > 1e-6).mean() < 1e-3
        return run, verify
    return build


for h_, w_ in IMAGE_SHAPES:
    add(Case(f"density_from_depth-{h_}x{w_}", ("awseg_fog_density_from_depth",), _density_from_depth(h_, w_),
             "oracle.cpu_oracle.fog_density_from_depth", "test_gpu_kernels.py::test_density_from_depth (1e-6 abs on 99.9 % of pixels)",
             sizes=("awseg_density_workspace",)))


# ================================================================================================================== loss
def _loss(shape, focal, ldt):
    def build(device):
        ops, oracle = _ops(), _oracle()
        rs = np.random.RandomState(1)
        x = (rs.randn(*shape) * 3).astype(np.float32)
        lab = rs.randint(0, shape[1], (shape[0],) + shape[2:]).astype(ldt)
        dens = rs.rand(shape[0], *shape[2:]).astype(np.float32)

        def run():
            oob = torch.full((1,), 5, dtype=torch.int64, device=device)
            mean, pix = ops.fog_ce_forward(_dev(x, device), _dev(lab, device), _dev(dens, device), focal, 2.0, oob, want_pixel=True)
            grad = ops.fog_ce_backward(_dev(x, device), _dev(lab, device), _dev(dens, device), focal, 2.0, torch.full((1,), 0.7, device=device))
            return {"mean": mean, "pixel_loss": pix, "grad_logits": grad, "oob": oob}

        def verify(r):
            ref_mean, ref_pix = oracle.fog_ce(x, lab.astype(np.uint8), dens, focal=focal, want_pixel=True)
            assert abs(r["mean"].item() - ref_mean) < 1e-5
            assert np.abs(_np(r["pixel_loss"]) - ref_pix).max() < 1e-4
            assert np.abs(_np(r["grad_logits"]) - oracle.fog_ce_grad(x, lab.astype(np.uint8), dens, focal=focal, g=0.7)).max() < 1e-6
            assert r["oob"].item() == 5
        return run, verify
    return build


_LOSS_GATE = "test_gpu_kernels.py::test_loss_vs_oracle (mean 1e-5, per pixel 1e-4, gradient 1e-6 abs)"
# one block per image: 5 x 7 (scalar lanes) and 8 x 16 (float4 lanes); two blocks per image (hw > launch_geometry.LOSS_THREADS):
# 13 x 20 (float4 lanes) and 7 x 37 (scalar lanes).  partials: exactly awseg_loss_partials doubles.
for shape_, ldt_ in [((2, 19, 5, 7), "uint8"), ((2, 19, 8, 16), "int64"), ((2, 19, 13, 20), "uint8"), ((2, 7, 7, 37), "int64")]:
    for focal_ in (False, True):
        add(Case(f"loss-{'focal' if focal_ else 'ce'}-{'x'.join(map(str, shape_))}-{ldt_}", ("awseg_fog_ce_forward", "awseg_fog_ce_backward"),
                 _loss(shape_, focal_, ldt_), "oracle.cpu_oracle.fog_ce / fog_ce_grad", _LOSS_GATE, sizes=("awseg_loss_partials",),
                 inout=("oob",)))
add(Case("loss-ce-2x19x5x7-out+4", ("awseg_fog_ce_forward", "awseg_fog_ce_backward"), _loss((2, 19, 5, 7), False, "uint8"),
         "oracle.cpu_oracle.fog_ce / fog_ce_grad", _LOSS_GATE, sizes=("awseg_loss_partials",), inout=("oob",),
         offsets={"pixel_loss": 4, "grad_logits": 4}))


for shape_ in [(2, 19, 8, 16), (2, 19, 13, 20)]:            # float4-eligible planes with logits, label and density one element off alignment
    add(Case(f"loss-ce-{'x'.join(map(str, shape_))}-inputs+1", ("awseg_fog_ce_forward", "awseg_fog_ce_backward"),
             _off_alignment(_loss(shape_, False, "uint8")), "oracle.cpu_oracle.fog_ce / fog_ce_grad", _LOSS_GATE, sizes=("awseg_loss_partials",),
             inout=("oob",), shifted=("logits", "density")))


# ======================================================================================= label-map and logit scanners: metrics
def _labels(rs, c, shape, ldt):
    lab = rs.randint(0, c, shape)
    lab[rs.rand(*shape) < 0.05] = 255
    return lab.astype(ldt)


def _confusion(c, hw, ldt):
    def build(device):
        ops, oracle = _ops(), _oracle()
        rs = np.random.RandomState(c + hw[0])
        n = 2 * hw[0] * hw[1]
        pred = rs.randint(0, c, n).astype(np.int64 if ldt == "int64" else np.uint8)
        lab = _labels(rs, c, (n,), ldt)

        def run():
            counts = torch.full((1, c * c), 3, dtype=torch.int64, device=device)
            oob = torch.full((1,), 2, dtype=torch.int64, device=device)
            ops.confusion_accumulate(_dev(pred, device), _dev(lab, device), c, counts, oob)
            return {"counts": counts, "oob": oob}

        def verify(r):
            assert np.array_equal(_np(r["counts"])[0], oracle.confusion(pred.astype(np.int64), lab, c) + 3) and r["oob"].item() == 2
        return run, verify
    return build


def _combine(c, hw, ldt, single):
    def build(device):
        ops, oracle = _ops(), _oracle()
        rs = np.random.RandomState(3)
        s1 = rs.randn(2, c, *hw).astype(np.float32)
        s2 = rs.randn(2, c, *hw).astype(np.float32)
        lab = _labels(rs, c, (2,) + hw, ldt)
        cond = np.array([1, 0], dtype=np.int32)

        def run():
            counts = torch.full((3, c * c), 3, dtype=torch.int64, device=device)
            oob = torch.full((1,), 2, dtype=torch.int64, device=device)
            w = torch.tensor([0.4, 0.6], device=device)
            t = torch.tensor([1.3], device=device)
            out, pred = ops.combine_argmax_confusion(_dev(s1, device), None if single else _dev(s2, device), 0, w, t, want_logits=True,
                                                     want_pred=True, pred_dtype=torch.uint8 if ldt == "uint8" else torch.int64,
                                                     label=_dev(lab, device), counts=counts, oob=oob, cond=_dev(cond, device))
            r = {"pred": pred, "counts": counts, "oob": oob}
            if not single:
                r["out_logits"] = out
            return r

        def verify(r):
            ref_logits = s1 if single else oracle.combine(s1, s2, 0, float(np.float32(0.4)), float(np.float32(0.6)), float(np.float32(1.3)))
            if not single:
                assert np.array_equal(_np(r["out_logits"]), ref_logits)
            ref_pred = oracle.argmax(ref_logits)
            assert np.array_equal(_np(r["pred"]).astype(np.int64), ref_pred)
            got = _np(r["counts"]) - 3
            assert np.array_equal(got[0], oracle.confusion(ref_pred, lab, c))
            for slot, b in ((1, 1), (2, 0)):
                assert np.array_equal(got[slot], oracle.confusion(ref_pred[b:b + 1], lab[b:b + 1], c))
            assert r["oob"].item() == 2
        return run, verify
    return build


def _argmax(c, hw, dt):
    def build(device):
        ops, oracle = _ops(), _oracle()
        rs = np.random.RandomState(sum(hw) + c)
        x = np.round(rs.randn(2, c, *hw).astype(np.float32) * 2) / 2

        def run():
            return {"pred": ops.argmax(_dev(x, device), dt)}

        def verify(r):
            assert np.array_equal(_np(r["pred"]).astype(np.int64), oracle.argmax(x))
        return run, verify
    return build


def _ece(c, hw, ldt):
    def build(device):
        ops, oracle = _ops(), _oracle()
        rs = np.random.RandomState(4)
        x = (rs.randn(2, c, *hw) * 3).astype(np.float32)
        lab = _labels(rs, c, (2,) + hw, ldt)

        def run():
            bins = ops.new_ece_bins(15, device, 3)
            bins[:, :, 0] += 2                                       # non-zero counts to accumulate onto
            ops.ece_accumulate(_dev(x, device), _dev(lab, device), bins, torch.linspace(0, 1, 16).to(device),
                               cond=torch.tensor([1, 0], dtype=torch.int32, device=device))
            return {"bins": bins}

        def verify(r):
            got = ops.ece_bins_to_numpy(r["bins"].clone())
            cnt, _, _ = oracle.ece_bins(x, lab.astype(np.uint8))
            # bin membership can differ from the oracle only where expf differs in the last ulp at an edge
            assert np.abs(got[0]["count"] - 2 - cnt).sum() <= 2
            assert np.array_equal(got[0]["count"] - 2, got[1]["count"] - 2 + got[2]["count"] - 2)
        return run, verify
    return build


_SCAN_GATE = "test_gpu_kernels.py::test_fused_combine_argmax_confusion_slots / test_confusion_vs_oracle_ragged (bit-exact)"
for c_ in (7, 19):
    for hw_ in MAP_SHAPES:
        for ldt_ in ("uint8", "int64"):
            tag_ = f"{c_}-{hw_[0]}x{hw_[1]}-{ldt_}"
            add(Case(f"confusion-{tag_}", ("awseg_confusion_accumulate",), _confusion(c_, hw_, ldt_), "oracle.cpu_oracle.confusion", _SCAN_GATE,
                     sizes=("awseg_metrics_workspace",), inout=("counts", "oob")))
            add(Case(f"combine-{tag_}", ("awseg_combine_argmax_confusion",), _combine(c_, hw_, ldt_, False),
                     "oracle.cpu_oracle.combine / argmax / confusion", _SCAN_GATE, sizes=("awseg_metrics_workspace",), inout=("counts", "oob")))
            add(Case(f"argmax_confusion-{tag_}", ("awseg_argmax_confusion",), _combine(c_, hw_, ldt_, True),
                     "oracle.cpu_oracle.argmax / confusion", _SCAN_GATE, sizes=("awseg_metrics_workspace",), inout=("counts", "oob")))
            add(Case(f"argmax-{tag_}", ("awseg_argmax",), _argmax(c_, hw_, torch.uint8 if ldt_ == "uint8" else torch.int64),
                     "oracle.cpu_oracle.argmax", "test_gpu_kernels.py::test_argmax_vs_oracle (bit-exact)"))
            add(Case(f"ece-{tag_}", ("awseg_ece_accumulate",), _ece(c_, hw_, ldt_), "oracle.cpu_oracle.ece_bins",
                     "test_gpu_kernels.py::test_ece_bins (at most 2 pixels change bin)", sizes=("awseg_metrics_workspace",), inout=("bins",)))
for hw_ in ((5, 7), (8, 16)):            # 8 x 16: hw % 16 == 0, so the alignment of the base alone selects the path
    add(Case(f"ece-19-{hw_[0]}x{hw_[1]}-uint8-inputs+1", ("awseg_ece_accumulate",), _off_alignment(_ece(19, hw_, "uint8")), "oracle.cpu_oracle.ece_bins",
             "test_gpu_kernels.py::test_ece_bins (at most 2 pixels change bin)", sizes=("awseg_metrics_workspace",), inout=("bins",),
             shifted=("logits", "label")))
add(Case("combine-19-5x7-uint8-out+1", ("awseg_combine_argmax_confusion",), _combine(19, (5, 7), "uint8", False),
         "oracle.cpu_oracle.combine / argmax / confusion", _SCAN_GATE, sizes=("awseg_metrics_workspace",), inout=("counts", "oob"),
         offsets={"pred": 1, "out_logits": 4}))
add(Case("argmax-19-5x7-uint8-out+1", ("awseg_argmax",), _argmax(19, (5, 7), torch.uint8), "oracle.cpu_oracle.argmax",
         "test_gpu_kernels.py::test_argmax_vs_oracle (bit-exact)", offsets={"pred": 1}))


# ================================================================================================================== GEMM family
def _gemm_inputs(m, n, k, device, seed=0):
    g = torch.Generator(device=device).manual_seed(m + n + k + seed)
    x = torch.randn(m, k, device=device, generator=g) * 2.0
    w = torch.randn(n, k, device=device, generator=g) * 0.05
    x[::7, ::3] *= 1e-5                                          # f16-subnormal high parts
    return x, w, torch.randn(n, device=device, generator=g), torch.randn(m, n, device=device, generator=g)


def _gemm_ref(x, w, bias, res, act):
    ref = x.double() @ w.double().t() + bias.double()
    if res is not None:
        ref = ref + res.double()
    return ref.clamp_min(0) if act else ref


def _gemm(kind, m, n, k, alias):
    """kind: 'library' (hipBLASLt float32), 'split', 'bf16'.  alias: the residual's buffer is the output."""
    def build(device):
        ops = _ops()
        x, w, bias, res = _gemm_inputs(m, n, k, device)
        ref = _gemm_ref(x, w, bias, res if alias else None, 1)

        def run():
            out = res.clone() if alias else None
            if kind == "library":
                return {"out": ops.gemm_bias_act(x, w, bias, 1, residual=out, out=out, split=False)}
            if kind == "split":
                ws = ops.gemm_split_weights(w)
                return {"out": ops.gemm_split_bias_act(x, ws, bias, 1, residual=out, out=out), "w_split": ws}
            wb = ops.gemm_bf16_weights(w)
            return {"out": ops.gemm_bf16_bias_act(x, wb, bias, 1, residual=out, out=out), "w_bf16": wb}

        def verify(r):
            err = (r["out"].double() - ref).abs()
            if kind == "library":
                assert err.max().item() < 1e-4
            elif kind == "split":
                assert err.max().item() < 1e-5 * max(1.0, ref.abs().max().item())
            else:
                exact = _gemm_ref(x.to(torch.bfloat16), w.to(torch.bfloat16), bias, res if alias else None, 1)
                rowmag = ref.abs().amax(dim=1).clamp_min(1.0)
                assert ((r["out"].double() - exact).abs().amax(dim=1) / rowmag).max().item() < 2e-5
                assert (err.amax(dim=1) / rowmag).max().item() < 2e-2
        return run, verify
    return build


_GEMM_SHAPES = [(128, 128, 64, False), (129, 128, 64, False), (200, 192, 72, False), (129, 192, 72, True), (200, 128, 64, True)]
for m_, n_, k_, alias_ in _GEMM_SHAPES:
    tag_ = f"{m_}x{n_}x{k_}{'-residual-is-out' if alias_ else ''}"
    add(Case(f"gemm-library-{tag_}", ("awseg_gemm_bias_act",), _gemm("library", m_, n_, k_, alias_), "float64 x @ w.T + bias (+ residual), ReLU",
             "test_gpu_kernels.py::test_gemm_bias_act_epilogues (1e-4 abs)", free_workspace=True))
    add(Case(f"gemm-split-{tag_}", ("awseg_gemm_split_weights", "awseg_gemm_split_bias_act"), _gemm("split", m_, n_, k_, alias_),
             "float64 x @ w.T + bias (+ residual), ReLU", "test_gpu_kernels.py::test_gemm_split_float32_grade (1e-5 of the largest output)",
             sizes=("awseg_gemm_split_weight_halfs",)))
    # the bf16 weight launcher fills plane 0, the trailer and the k-blocked image; plane 1 is documented unused and never written
    add(Case(f"gemm-bf16-{tag_}", ("awseg_gemm_bf16_weights", "awseg_gemm_bf16_bias_act"), _gemm("bf16", m_, n_, k_, alias_),
             "float64 on bf16-rounded operands, and unrounded float64", "test_gpu_bf16.py::test_gemm_bf16 (2e-5 / 2e-2 of the row's largest output)",
             sizes=("awseg_gemm_bf16_weight_halfs",), partial=("w_bf16",)))


# ==================================================================================================================== attention
def _attention(kind, b, heads, nq, nkv):
    """kind: f32 | split | split_ws | packed0 | packed1 | packed2 | bf16"""
    def build(device):
        ops = _ops()
        g = torch.Generator(device=device).manual_seed(b + heads + nq + nkv)
        c = heads * 32
        q = torch.randn(b, nq, c, device=device, generator=g)
        kv = torch.randn(b, nkv, 2 * c, device=device, generator=g)
        k, v = kv[..., :c].contiguous(), kv[..., c:].contiguous()
        scale = 32 ** -0.5
        qh, kh, vh = (t.double().view(b, -1, heads, 32).transpose(1, 2) for t in (q, k, v))
        ref = (torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1) @ vh).transpose(1, 2).reshape(b, nq, c) if nkv % 32 == 0 else None

        def run():
            N = ops.N
            if nkv % 32:                                            # whole key tiles only: the launcher declines, nothing is written
                out = torch.empty_like(q)
                sym = {"f32": "awseg_attention_d32", "split": "awseg_attention_d32_split", "bf16": "awseg_attention_d32_bf16"}[kind]
                N.try_call(sym, N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(out), b, heads, nq, nkv, float(scale), N.stream())
                return {"out": out}
            if kind in ("f32", "split"):
                return {"out": ops.attention_d32(q, k, v, heads, scale, split=kind == "split")}
            if kind == "split_ws":
                out = torch.empty_like(q)
                ops._attention_split_ws(q, k, v, 0, out, b, heads, nq, nkv, scale)
                return {"out": out}
            if kind == "packed_ws":
                out = torch.empty_like(q)
                ops._attention_split_ws(q, kv, kv[..., c:], 2 * c, out, b, heads, nq, nkv, scale)
                return {"out": out}
            if kind == "bf16":
                with ops.precision("bf16"):
                    return {"out": ops.attention_d32(q, k, v, heads, scale)}
            out = torch.empty_like(q)
            N.call("awseg_attention_d32_packed_kv", N.ptr(q), N.ptr(kv), N.ptr(out), b, heads, nq, nkv, float(scale), int(kind[-1]), N.stream())
            return {"out": out}

        def verify(r):
            if ref is not None:
                assert (r["out"].double() - ref).abs().max().item() < (3e-2 if kind in ("bf16", "packed2") else 2e-5)
        return run, verify
    return build


_ATTN_GATE = "test_gpu_kernels.py::test_attention_d32_matches_sdpa / _split_operands_float32_grade (2e-5 abs); test_gpu_bf16.py::test_attention_d32_bf16 (3e-2 abs)"
_ATTN_SYM = {"f32": "awseg_attention_d32", "split": "awseg_attention_d32_split", "split_ws": "awseg_attention_d32_split_ws",
             "packed_ws": "awseg_attention_d32_split_ws", "packed0": "awseg_attention_d32_packed_kv", "packed1": "awseg_attention_d32_packed_kv",
             "packed2": "awseg_attention_d32_packed_kv", "bf16": "awseg_attention_d32_bf16"}
for kind_ in _ATTN_SYM:
    for b_, heads_, nq_, nkv_ in [(2, 1, 33, 32), (1, 2, 160, 96), (2, 2, 33, 96), (1, 1, 160, 32)]:
        add(Case(f"attention-{kind_}-b{b_}-h{heads_}-q{nq_}-k{nkv_}", (_ATTN_SYM[kind_],), _attention(kind_, b_, heads_, nq_, nkv_),
                 "float64 softmax(q k^T scale) v", _ATTN_GATE, sizes=("awseg_attention_d32_split_workspace",) if kind_.endswith("_ws") else ()))
for kind_ in ("f32", "split", "bf16"):                            # 40 keys: not a multiple of the 32-key tile -> AWSEG_ERANGE
    add(Case(f"attention-{kind_}-b1-h1-q33-k40-declined", (_ATTN_SYM[kind_],), _attention(kind_, 1, 1, 33, 40), "float64 softmax(q k^T scale) v",
             _ATTN_GATE, declines={_ATTN_SYM[kind_]: -2}, partial=("out",)))


# ========================================================= small operators around the backbones (off-grid maps, one or two tiles)
def _simple(make):
    """make(device, ops) -> (inputs..., run, verify) helpers below share this shape: seeded inputs made once per build."""
    def build(device):
        return make(device, _ops())
    return build


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _layernorm(rows, c):
    def make(device, ops):
        g = _gen(device, c)
        x = torch.randn(rows, c, device=device, generator=g) * 3 + 1
        ga, be = torch.randn(c, device=device, generator=g), torch.randn(c, device=device, generator=g)
        ref = torch.nn.functional.layer_norm(x.double(), (c,), ga.double(), be.double(), 1e-5)
        return (lambda: {"out": ops.layernorm_rows(x, ga, be, 1e-5)}), (lambda r: _lt((r["out"].double() - ref).abs().max().item(), 2e-5))
    return _simple(make)


def _lt(value, bound):
    assert value < bound, f"{value:.3e} is not below {bound:.1e}"


for rows_, c_ in [(33, 4), (130, 32), (33, 160), (130, 64)]:
    add(Case(f"layernorm-{rows_}x{c_}", ("awseg_layernorm_rows",), _layernorm(rows_, c_), "float64 layer_norm",
             "test_gpu_kernels.py::test_layernorm_rows (2e-5 abs)"))


def _dwconv(b, h, w, c, act, dil, bias):
    def make(device, ops):
        g = _gen(device, h * w + c)
        x = torch.randn(b, c, h, w, device=device, generator=g)
        wt = torch.randn(c, 1, 3, 3, device=device, generator=g)
        bi = torch.randn(c, device=device, generator=g) if bias else None
        ref = torch.nn.functional.conv2d(x, wt, bi, padding=dil, dilation=dil, groups=c)
        ref = {0: ref, 1: torch.relu(ref), 2: torch.nn.functional.gelu(ref)}[act]
        xl, w9 = x.permute(0, 2, 3, 1).contiguous(), wt.view(c, 9).t().contiguous()
        return (lambda: {"out": ops.dwconv3x3_nhwc(xl, w9, bi, act, dilation=dil)}), \
            (lambda r: _lt((r["out"].permute(0, 3, 1, 2) - ref).abs().max().item(), 1e-5))
    return _simple(make)


for b_, h_, w_, c_, act_, dil_, bias_ in [(2, 33, 35, 4, 0, 1, True), (1, 40, 72, 8, 2, 1, True), (2, 1, 9, 4, 1, 1, False), (1, 33, 35, 4, 1, 3, False),
                                          (2, 16, 32, 4, 0, 1, True)]:
    add(Case(f"dwconv-{b_}x{h_}x{w_}x{c_}-act{act_}-d{dil_}", ("awseg_dwconv3x3_nhwc",), _dwconv(b_, h_, w_, c_, act_, dil_, bias_),
             "torch conv2d(groups=C) (+ GELU / ReLU)", "test_gpu_kernels.py::test_dwconv3x3_nhwc_and_bias_act (1e-5 abs)"))


def _bias_act(n, c, res, act):
    def make(device, ops):
        g = _gen(device, n + c)
        y = torch.randn(n, c, device=device, generator=g)
        r_ = torch.randn(n, c, device=device, generator=g) if res else None
        b_ = torch.randn(c, device=device, generator=g)
        want = y + b_ + r_ if res else y + b_
        want = torch.relu(want) if act else want
        return (lambda: {"x": ops.bias_act_nhwc_(y.clone(), b_, r_, act)}), (lambda r: _eq(r["x"], want))
    return _simple(make)


def _eq(a, b):
    assert torch.equal(a, b)


for n_, c_, res_, act_ in [(33, 4, True, 1), (130, 8, False, 0), (128, 64, True, 1)]:
    add(Case(f"bias_act-{n_}x{c_}-res{int(res_)}-act{act_}", ("awseg_bias_act_nhwc",), _bias_act(n_, c_, res_, act_), "torch relu(x + bias + residual)",
             "test_gpu_kernels.py::test_dwconv3x3_nhwc_and_bias_act (bit-exact)", inout=("x",)))


def _maxpool(b, h, w, c, shift):
    def make(device, ops):
        g = _gen(device, h + w + c)
        x = torch.randn(b, h, w, c, device=device, generator=g)
        sh = torch.randn(c, device=device, generator=g) if shift else None
        ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        if shift:
            ref = torch.relu(ref + sh)
        return (lambda: {"out": ops.maxpool3x3s2_nhwc(x, shift=sh)}), (lambda r: _eq(r["out"], ref))
    return _simple(make)


for b_, h_, w_, c_ in [(2, 33, 35, 4), (1, 40, 72, 8), (2, 16, 32, 4), (1, 1, 7, 12)]:
    add(Case(f"maxpool-{b_}x{h_}x{w_}x{c_}", ("awseg_maxpool3x3s2_nhwc",), _maxpool(b_, h_, w_, c_, False), "torch max_pool2d(3, 2, 1)",
             "test_gpu_kernels.py::test_maxpool3x3s2_nhwc_equals_torch (bit-exact)"))
    add(Case(f"maxpool-bias-relu-{b_}x{h_}x{w_}x{c_}", ("awseg_maxpool3x3s2_bias_relu_nhwc",), _maxpool(b_, h_, w_, c_, True),
             "torch relu(max_pool2d(3, 2, 1) + shift)", "test_gpu_kernels.py::test_maxpool3x3s2_nhwc_equals_torch (bit-exact)"))


def _upsample(b, c, h, w, H, W, align, entry):
    def make(device, ops):
        g = _gen(device, h * w)
        x = torch.randn(b, c, h, w, device=device, generator=g)
        ref = torch.nn.functional.interpolate(x, size=(H, W), mode="bilinear", align_corners=align)

        def run():
            if entry == "strided":
                return {"out": ops.upsample_bilinear(x, (H, W), align)}
            N = ops.N
            out = torch.empty(b, c, H, W, device=device)
            N.call("awseg_upsample_bilinear", N.ptr(x), b * c, h, w, H, W, int(align), N.ptr(out), N.stream())
            return {"out": out}
        return run, (lambda r: _lt((r["out"] - ref).abs().max().item(), 1e-6 * max(1.0, ref.abs().max().item())))
    return _simple(make)


for cfg_ in [(2, 1, 4, 8, 64, 128, False), (1, 2, 5, 9, 33, 70, False), (1, 3, 7, 5, 28, 20, True), (1, 2, 9, 12, 18, 24, True), (1, 1, 6, 6, 5, 4, True),
             (2, 2, 9, 9, 33, 35, False)]:
    for entry_ in ("planar", "strided"):
        add(Case(f"upsample-{entry_}-{'x'.join(map(str, cfg_[:6]))}-align{int(cfg_[6])}",
                 ("awseg_upsample_bilinear" if entry_ == "planar" else "awseg_upsample_bilinear_strided",), _upsample(*cfg_, entry_),
                 "torch F.interpolate(bilinear)", "test_gpu_kernels.py::test_upsample_bilinear_matches_torch (1e-6 of the largest output)"))


def _upcat(b, h, w, ca, ch):
    def make(device, ops):
        g = _gen(device, b + h + w + ca + ch)
        a = torch.randn(b, ca, h, w, device=device, generator=g)
        hi = torch.randn(b, ch, 4 * h, 4 * w, device=device, generator=g)
        wdw = torch.randn(ca + ch, 1, 3, 3, device=device, generator=g)
        cat = torch.cat([torch.nn.UpsamplingBilinear2d(scale_factor=4)(a), hi], dim=1)
        ref = torch.nn.functional.conv2d(cat, wdw, padding=1, groups=ca + ch)
        al, hl, w9 = a.permute(0, 2, 3, 1).contiguous(), hi.permute(0, 2, 3, 1).contiguous(), wdw.view(ca + ch, 9).t().contiguous()
        return (lambda: {"out": ops.dwconv3x3_upcat(al, hl, w9)}), (lambda r: _lt((r["out"].permute(0, 3, 1, 2) - ref).abs().max().item(), 1e-5))
    return _simple(make)


for shape_ in [(2, 5, 7, 8, 4), (1, 3, 3, 4, 4), (2, 9, 13, 256, 8), (1, 8, 9, 4, 4)]:
    add(Case(f"upcat-{'x'.join(map(str, shape_))}", ("awseg_dwconv3x3_upcat_nhwc",), _upcat(*shape_), "torch conv2d(cat(UpsamplingBilinear2d(a), hi))",
             "test_gpu_kernels.py::test_dwconv3x3_upcat_matches_torch (1e-5 abs)"))


def _aspp(b, h, w, c, rates, mean):
    def make(device, ops):
        g = _gen(device, b + h + w + c)
        x = torch.randn(b, c, h, w, device=device, generator=g)
        wdw = torch.randn(3, c, 1, 3, 3, device=device, generator=g)
        xl, wl = x.permute(0, 2, 3, 1).contiguous(), wdw.reshape(3, c, 9).permute(0, 2, 1).contiguous()

        def run():
            if not mean:
                return {"out": ops.aspp_depthwise3(xl, wl, rates)}
            out, m = ops.aspp_depthwise3_mean(xl, wl, rates)
            return {"out": out, "mean_out": m}

        def verify(r):
            for i in range(3):
                ref = torch.nn.functional.conv2d(x, wdw[i], padding=rates[i], dilation=rates[i], groups=c)
                _lt((r["out"][i].permute(0, 3, 1, 2) - ref).abs().max().item(), 1e-4)
            if mean:
                _lt((r["mean_out"].double() - xl.double().mean(dim=(1, 2))).abs().max().item(), 1e-6)
        return run, verify
    return _simple(make)


_ASPP_GATE = "test_gpu_kernels.py::test_aspp_depthwise3 / _xcd_sliced_path / _with_mean_output (1e-4 abs; mean 1e-6)"
for b_, h_, w_, c_, rates_ in [(2, 20, 28, 16, (3, 6, 9)), (3, 10, 7, 64, (12, 24, 36)), (1, 33, 35, 4, (3, 6, 9)), (2, 16, 24, 64, (3, 5, 7))]:
    add(Case(f"aspp-{b_}x{h_}x{w_}x{c_}", ("awseg_aspp_depthwise3",), _aspp(b_, h_, w_, c_, rates_, False), "torch dilated conv2d(groups=C)", _ASPP_GATE))
for b_, h_, w_, c_, rates_ in [(2, 16, 24, 64, (3, 5, 7)), (3, 9, 8, 32, (12, 24, 36)), (1, 33, 35, 32, (3, 6, 9))]:
    add(Case(f"aspp-mean-{b_}x{h_}x{w_}x{c_}", ("awseg_aspp_depthwise3_mean",), _aspp(b_, h_, w_, c_, rates_, True),
             "torch dilated conv2d(groups=C); float64 mean", _ASPP_GATE))


def _rowdot(rows, k, sigmoid):
    def make(device, ops):
        g = _gen(device, rows + k)
        x = torch.randn(rows, k, device=device, generator=g)
        w = torch.randn(k, device=device, generator=g) * 0.1
        b = torch.randn(1, device=device, generator=g) if sigmoid else None
        ref = torch.sigmoid(x.double() @ w.double() + b.double()) if sigmoid else x.double() @ w.double()
        return (lambda: {"out": ops.rowdot_sigmoid(x, w, b, sigmoid=sigmoid)}), \
            (lambda r: _lt((r["out"].double() - ref).abs().max().item(), 1e-6 if sigmoid else 1e-5))
    return _simple(make)


for rows_, k_, sg_ in [(33, 4, True), (130, 128, True), (130, 12, False)]:
    add(Case(f"rowdot-{rows_}x{k_}-sigmoid{int(sg_)}", ("awseg_rowdot_sigmoid",), _rowdot(rows_, k_, sg_), "float64 sigmoid(x @ w + b)",
             "test_gpu_kernels.py::test_rowdot_sigmoid_and_aspp_pool_branch_vs_float64 (1e-6 / 1e-5 abs)"))


def _pool_branch(batch, cin, cmid, cout, b2):
    def make(device, ops):
        g = _gen(device, batch + cin)
        mean = torch.randn(batch, cin, device=device, generator=g)
        w1 = torch.randn(cmid, cin, device=device, generator=g) / cin ** 0.5
        b1 = torch.randn(cmid, device=device, generator=g)
        w2 = torch.randn(cout, cmid, device=device, generator=g) / cmid ** 0.5
        bb = torch.randn(cout, device=device, generator=g) if b2 else None
        ref = torch.relu(mean.double() @ w1.double().t() + b1.double()) @ w2.double().t() + (bb.double() if b2 else 0)
        return (lambda: {"out": ops.aspp_pool_branch(mean, w1, b1, w2, bb)}), (lambda r: _lt((r["out"].double() - ref).abs().max().item(), 2e-5))
    return _simple(make)


for cfg_ in [(11, 520, 30, 19, True), (2, 64, 256, 256, False), (1, 33, 5, 3, True)]:
    add(Case(f"aspp_pool_branch-{'x'.join(map(str, cfg_[:4]))}", ("awseg_aspp_pool_branch",), _pool_branch(*cfg_), "float64 relu(mean w1^T + b1) w2^T + b2",
             "test_gpu_kernels.py::test_rowdot_sigmoid_and_aspp_pool_branch_vs_float64 (2e-5 abs)", sizes=("awseg_aspp_pool_branch_workspace",)))


def _stem_image(b, c, h, w, cl):
    def make(device, ops):
        g = _gen(device, 3)
        x = torch.randn(b, c, h, w, device=device, generator=g)
        if cl:
            x = x.contiguous(memory_format=torch.channels_last)
        wp = w + 11
        ref = torch.full((b, h, wp, 4), 7.0, device=device)
        ref[:, :, 3:3 + w, :c] = x.permute(0, 2, 3, 1)
        if c < 4:
            ref[:, :, 3:3 + w, c:] = 0.0

        def run():
            got = torch.full((b, h, wp, 4), 7.0, device=device)
            ops.stem_image_fill(x, got)
            return {"image": got}
        return run, (lambda r: _eq(r["image"], ref))
    return _simple(make)


for cfg_ in [(2, 3, 9, 37, False), (1, 3, 8, 64, True), (2, 4, 5, 16, False)]:
    add(Case(f"stem_image-{'x'.join(map(str, cfg_[:4]))}{'-cl' if cfg_[4] else ''}", ("awseg_stem_image",), _stem_image(*cfg_),
             "torch strided copy into the padded image", "test_gpu_kernels.py::test_stem_image_fill_matches_strided_copy (bit-exact)",
             inout=("image",)))            # the caller zeroed the padding once: cells outside the interior keep what they hold


def _depth_up(b, h, w, H, W, weighted):
    def make(device, ops):
        g = _gen(device, b + h + w + H + W)
        d1 = torch.rand(b, 1, H, W, device=device, generator=g)
        lo = torch.rand(b, 1, h, w, device=device, generator=g)
        wts = torch.softmax(torch.tensor([0.3, -0.2], device=device), 0) if weighted else None
        ref2 = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
        ref = wts[0] * d1 + wts[1] * ref2 if weighted else (d1 + ref2) / 2

        def run():
            d2, d = ops.depth_upsample_combine(d1, lo, wts)
            return {"d2_full": d2, "d_out": d}
        return run, (lambda r: (_lt((r["d2_full"] - ref2).abs().max().item(), 1e-6), _lt((r["d_out"] - ref).abs().max().item(), 1e-6)))
    return _simple(make)


for cfg_ in [(2, 4, 8, 64, 128, True), (1, 3, 5, 37, 61, True), (2, 3, 3, 33, 35, False)]:
    add(Case(f"depth_upsample_combine-{'x'.join(map(str, cfg_[:5]))}-w{int(cfg_[5])}", ("awseg_depth_upsample_combine",), _depth_up(*cfg_),
             "torch F.interpolate + weighted sum", "test_gpu_kernels.py::test_depth_upsample_combine_matches_torch (1e-6 abs)"))


def _im2col(b, h, w, c, kh, kw, s, p):
    def make(device, ops):
        import torch.nn.functional as F
        g = _gen(device, b + h + w + c + kh)
        x = torch.randn(b, h, w, c, device=device, generator=g)
        kp = (kh * kw * c + 7) // 8 * 8

        def verify(r):
            cols = r["cols"]
            ho, wo = (h + 2 * p - kh) // s + 1, (w + 2 * p - kw) // s + 1
            un = F.unfold(x.permute(0, 3, 1, 2), (kh, kw), dilation=1, padding=p, stride=s)
            un = un.view(b, c, kh * kw, ho * wo).permute(0, 3, 2, 1).reshape(b * ho * wo, kh * kw * c)
            assert torch.equal(cols[:, :kh * kw * c], un) and (cols[:, kh * kw * c:] == 0).all()
        return (lambda: {"cols": ops.im2col_nhwc(x, kh, kw, s, p, 1, kp)[0]}), verify
    return _simple(make)


for cfg_ in [(2, 17, 23, 8, 3, 3, 2, 1), (1, 9, 11, 4, 3, 3, 2, 1), (2, 16, 20, 32, 2, 2, 2, 0), (1, 33, 35, 4, 3, 3, 2, 1)]:
    add(Case(f"im2col-{'x'.join(map(str, cfg_))}", ("awseg_im2col_nhwc",), _im2col(*cfg_), "torch F.unfold",
             "test_gpu_kernels.py::test_im2col_patch_gemm_is_the_convolution (bit-exact)"))


# ============================================================== label-map scanners (two frames, two condition slots, pre-filled counters)
def _label_maps(seed, c, h, w, ldt):
    """pred uint8, clean twin uint8, label [2, h, w]: labels mostly equal to the twin, about 5 % 255."""
    rs = np.random.RandomState(seed)
    ref = rs.randint(0, c, (2, h, w))
    ref[0] = np.repeat(np.repeat(ref[0, ::2, ::2], 2, 0), 2, 1)[:h, :w]       # frame 0 in 2 x 2 blocks: segments and bands exist
    pred = np.where(rs.rand(2, h, w) < 0.3, rs.randint(0, c, (2, h, w)), ref)
    lab = np.where(rs.rand(2, h, w) < 0.5, ref, rs.randint(0, c, (2, h, w)))
    lab[rs.rand(2, h, w) < 0.05] = 255
    return pred.astype(np.uint8), ref.astype(np.uint8), lab.astype(ldt)


COND = [1, 0]                                                          # frame 0 into slot 2, frame 1 into slot 1; slot 0 takes both
FILL = 3                                                               # what every accumulator holds before the call


def _prefilled(t):
    return t.add_(FILL)


def _i32(v, device):
    return torch.tensor(list(v), dtype=torch.int32, device=device)


def _consistency(c, h, w, ldt):
    def build(device):
        from tests import paired_ref as PR
        ops = _ops()
        pred, ref, lab = _label_maps(11, c, h, w, ldt)
        rows = ref[::-1].copy()

        def run():
            st, oob = _prefilled(ops.new_consistency_stats(c, device, 3)), torch.full((1,), FILL, dtype=torch.int64, device=device)
            ops.prediction_consistency(_dev(pred, device), _dev(rows, device), _i32([1, 0], device), _dev(lab, device), c, st, oob, _i32(COND, device))
            return {"stats": st, "oob": oob}

        def verify(r):
            want, bad = PR.consistency_stats(pred, [rows[1], rows[0]], lab, c, cond=COND, n_slots=3)
            assert np.array_equal(_np(r["stats"]) - FILL, want) and r["oob"].item() - FILL == bad
        return run, verify
    return build


def _boundary(c, h, w, ldt):
    def build(device):
        from tests import boundary_ref as BR
        ops = _ops()
        pred, _, lab = _label_maps(7, c, h, w, ldt)
        widths = (1, 2)

        def run():
            st, oob = _prefilled(ops.new_boundary_stats(c, len(widths), device, 3)), torch.full((1,), FILL, dtype=torch.int64, device=device)
            ops.boundary_stats(_dev(pred, device), _dev(lab, device), list(widths), c, st, oob, _i32(COND, device))
            return {"stats": st, "oob": oob}

        def verify(r):
            want, bad = BR.boundary_counters(pred, lab, widths, c, cond=COND, n_slots=3)
            assert np.array_equal(_np(r["stats"]) - FILL, want) and r["oob"].item() - FILL == bad
        return run, verify
    return build


def _segments(c, h, w, ldt):
    def build(device):
        from tests import segments_ref as SR
        ops = _ops()
        pred, ref, lab = _label_maps(5, c, h, w, ldt)

        def run():
            st, oob = _prefilled(ops.new_segment_stats(c, device, 3)), torch.full((1,), FILL, dtype=torch.int64, device=device)
            lid = torch.empty((2, h, w), dtype=torch.int32, device=device)
            pid = torch.empty((2, h, w), dtype=torch.int32, device=device)
            ops.segment_stats(_dev(pred, device), _dev(lab, device), c, st, oob, _i32(COND, device), ref_maps=_dev(ref, device),
                              frame_ref=_i32([0, 1], device), label_ids=lid, pred_ids=pid)
            return {"stats": st, "oob": oob, "label_ids": lid, "pred_ids": pid}

        def verify(r):
            want, bad, wl, wp = SR.segment_counters(pred, lab, c, cond=COND, n_slots=3, ref_maps=ref, frame_ref=[0, 1])
            assert np.array_equal(_np(r["stats"]) - FILL, want) and r["oob"].item() - FILL == bad
            assert np.array_equal(_np(r["label_ids"]), wl) and np.array_equal(_np(r["pred_ids"]), wp)
        return run, verify
    return build


def _frame_iou(c, h, w, ldt):
    def build(device):
        from tests import bootstrap_ref as BR
        ops = _ops()
        pred, _, lab = _label_maps(9, c, h, w, ldt)

        def run():
            table, oob = _prefilled(ops.new_frame_counts(3, c, device)), torch.full((1,), FILL, dtype=torch.int64, device=device)
            ops.frame_iou_counts(_dev(pred, device), _dev(lab, device), c, _i32([2, 0], device), table, oob)
            return {"table": table, "oob": oob}

        def verify(r):
            want, bad = BR.frame_counts(pred, lab, c, [2, 0], 3)
            assert np.array_equal(_np(r["table"]) - FILL, want) and r["oob"].item() - FILL == bad
        return run, verify
    return build


def _bootstrap(n, v, width):
    def build(device):
        from tests import bootstrap_ref as BR
        ops = _ops()
        rs = np.random.RandomState(n + v)
        table = rs.randint(0, 1000, (n, v, width)).astype(np.int64)
        slots = rs.randint(0, v + 1, (n, v)).astype(np.int32)

        def run():
            oob = torch.full((1,), FILL, dtype=torch.int64, device=device)
            return {"out": ops.bootstrap_counts(_dev(table, device), _dev(slots, device), 1 + v, 11, 7, oob, r0=3), "oob": oob}

        def verify(r):
            assert np.array_equal(_np(r["out"]), BR.replicate_sums(table, slots, 1 + v, 11, 3, 7))
            assert r["oob"].item() - FILL == BR.slot_oob(slots, 1 + v)
        return run, verify
    return build


def _change_strata(ch, h, w):
    def build(device):
        from tests import strata_ref as SR
        ops = _ops()
        rs = np.random.RandomState(5)
        clean = rs.rand(2, ch, h * w).astype(np.float32)
        var = (clean[::-1] + rs.rand(2, ch, h * w) * 0.4 * (rs.rand(2, 1, h * w) < 0.5)).astype(np.float32)
        edges = [0.02, 0.05, 0.1, 0.2]
        scale = None if ch == 3 else [0.25 * 255] * ch

        def run():
            oob = torch.full((1,), FILL, dtype=torch.int64, device=device)
            got = ops.change_strata(_dev(var.reshape(2, ch, h, w), device), _dev(clean.reshape(2, ch, h, w), device), _i32([1, 0], device),
                                    edges, scale=scale, oob=oob)
            return {"out": got, "oob": oob}

        def verify(r):
            want, bad = SR.change_strata(var, clean, [1, 0], edges, scale=scale)
            assert np.array_equal(_np(r["out"]).reshape(2, -1), want) and r["oob"].item() - FILL == bad
        return run, verify
    return build


def _stratified(c, h, w, ldt):
    def build(device):
        from tests import strata_ref as SR
        ops = _ops()
        pred, ref, lab = _label_maps(13, c, h, w, ldt)
        K = 5
        stratum = np.random.RandomState(2).randint(0, K, (2, h, w)).astype(np.uint8)

        def run():
            st, oob = _prefilled(ops.new_strata_stats(c, K, device, 3)), torch.full((1,), FILL, dtype=torch.int64, device=device)
            ops.stratified_stats(_dev(pred, device), _dev(lab, device), _dev(stratum, device), K, c, st, oob, ref_maps=_dev(ref, device),
                                 frame_ref=_i32([0, 1], device), cond=_i32(COND, device))
            return {"stats": st, "oob": oob}

        def verify(r):
            flat = lambda a: a.reshape(2, -1)                                             # noqa: E731
            want, bad = SR.stratified_stats(flat(pred), flat(lab), flat(stratum), K, c, refs=flat(ref), frame_ref=[0, 1], cond=COND, n_slots=3)
            assert np.array_equal(_np(r["stats"]) - FILL, want) and r["oob"].item() - FILL == bad
        return run, verify
    return build


def _weightgrid(hw, ldt):
    def build(device):
        from tests import weightgrid_ref as WR
        ops = _ops()
        s1, s2, lab = WR.eighths_case(100 + hw, 2, hw, np.dtype(ldt).type)
        grid = np.array([[0, 1], [0.25, 0.75], [0.5, 0.5], [1, 0]], np.float32)

        def run():
            st = _prefilled(ops.new_weight_grid_stats(3, len(grid), 19, device))
            ops.ensemble_weight_grid_stats(_dev(s1, device), _dev(s2, device), grid, _dev(lab, device), _i32(COND, device), st)
            return {"stats": st}

        def verify(r):
            want = WR.counters(s1, s2, grid, lab, cond=COND, n_slots=3)
            assert np.array_equal(_np(r["stats"]).reshape(want.shape) - FILL, want)
        return run, verify
    return build


_MAP_FAMILIES = [
    ("consistency", "awseg_prediction_consistency", _consistency, "awseg_consistency_workspace", "tests/paired_ref.py consistency_stats",
     "test_gpu_paired.py::test_consistency_counts_equal_numpy (bit-exact)"),
    ("boundary", "awseg_boundary_stats", _boundary, "awseg_boundary_workspace", "tests/boundary_ref.py boundary_counters",
     "test_gpu_boundary.py::test_counters_equal_the_model (bit-exact)"),
    ("segments", "awseg_segment_stats", _segments, "awseg_segment_workspace", "tests/segments_ref.py segment_counters",
     "test_gpu_segments.py check() (bit-exact counters and id maps)"),
    ("frame_iou", "awseg_frame_iou_counts", _frame_iou, "awseg_frame_iou_workspace", "tests/bootstrap_ref.py frame_counts",
     "test_gpu_bootstrap.py frame-count tests (bit-exact)"),
    ("stratified", "awseg_stratified_stats", _stratified, "awseg_strata_workspace", "tests/strata_ref.py stratified_stats",
     "test_gpu_strata.py::test_stratified_stats_equal_the_model (bit-exact)"),
]
for fam_, sym_, make_, size_, ref_, gate_ in _MAP_FAMILIES:
    for c_ in (7, 19):
        for hw_ in MAP_SHAPES:
            for ldt_ in ("uint8", "int64"):
                add(Case(f"{fam_}-{c_}-{hw_[0]}x{hw_[1]}-{ldt_}", (sym_,), make_(c_, hw_[0], hw_[1], ldt_), ref_, gate_, sizes=(size_,),
                         inout=("stats", "oob", "table")))
    for hw_ in ((5, 7), (8, 16)):            # inputs one element off alignment: the byte-load paths; at 8 x 16 alignment alone decides
        add(Case(f"{fam_}-19-{hw_[0]}x{hw_[1]}-uint8-inputs+1", (sym_,), _off_alignment(make_(19, hw_[0], hw_[1], "uint8")), ref_, gate_,
                 sizes=(size_,), inout=("stats", "oob", "table"), shifted=("pred", "label")))
for n_, v_, wd_ in [(1, 1, 57), (5, 13, 57), (64, 1, 21)]:
    add(Case(f"bootstrap-n{n_}-v{v_}-w{wd_}", ("awseg_bootstrap_counts",), _bootstrap(n_, v_, wd_), "tests/bootstrap_ref.py replicate_sums",
             "test_gpu_bootstrap.py::test_replicate_sums_equal_the_model (bit-exact)", inout=("oob",)))
for ch_, (h_, w_) in [(3, MAP_SHAPES[0]), (3, MAP_SHAPES[1]), (3, MAP_SHAPES[2]), (1, MAP_SHAPES[0])]:
    add(Case(f"change_strata-{ch_}x{h_}x{w_}", ("awseg_change_strata",), _change_strata(ch_, h_, w_), "tests/strata_ref.py change_strata",
             "test_gpu_strata.py::test_change_strata_equals_the_model (bit-exact)", inout=("oob",)))
add(Case("change_strata-3x5x7-out+1", ("awseg_change_strata",), _change_strata(3, 5, 7), "tests/strata_ref.py change_strata",
         "test_gpu_strata.py::test_change_strata_equals_the_model (bit-exact)", inout=("oob",), offsets={"out": 1}))
for hw_ in (36, 60, 128):            # the launcher has no scalar path: hw % 4 != 0 is AWSEG_EALIGN (5 x 7 is replaced by 6 x 6)
    for ldt_ in ("uint8", "int64"):
        add(Case(f"weightgrid-19-{hw_}-{ldt_}", ("awseg_ensemble_weight_grid_stats",), _weightgrid(hw_, ldt_), "tests/weightgrid_ref.py counters",
                 "test_gpu_weightgrid.py counters tests (bit-exact)", inout=("stats",)))


# ============================================================================================== Winograd 3x3 (float32, split, bf16)
def _winograd(kind, shape, variant):
    """variant: 'plain' (act 0), 'residual' (ReLU + residual), 'head' (fused 1x1 + sigmoid, Cout 64)"""
    def make(device, ops):
        b, h, w, cin, cout, d = shape
        g = _gen(device, sum(shape) + 17)
        x = torch.randn(b, h, w, cin, device=device, generator=g)
        wt = torch.randn(cout, cin, 3, 3, device=device, generator=g) / (3.0 * cin ** 0.5)
        scale = torch.rand(cout, device=device, generator=g) + 0.5
        shift = torch.randn(cout, device=device, generator=g)
        res = torch.randn(b, h, w, cout, device=device, generator=g)
        w2 = torch.randn(64, device=device, generator=g) * 0.2
        b2 = torch.randn(1, device=device, generator=g)
        ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), (wt * scale.view(-1, 1, 1, 1)).double(), None, 1, d, d)
        ref = ref.permute(0, 2, 3, 1) + shift.double()
        want = {"plain": lambda: ref, "residual": lambda: (ref + res.double()).clamp_min(0),
                "head": lambda: torch.sigmoid((ref.clamp_min(0) * w2.double()).sum(-1) + b2.double())}[variant]()
        kw = {"plain": dict(act=0), "residual": dict(act=1, residual=res), "head": dict(w2=w2, b2=b2)}[variant]
        u = {"f32": ops.winograd_weights, "split": ops.winograd_split_weights, "bf16": ops.winograd_bf16_weights}[kind](wt, scale)

        def run():
            if kind == "f32":
                return {"out": ops.conv3x3_winograd(x, u, shift, dilation=d, **kw)}
            fn = ops.conv3x3_winograd_split if kind == "split" else ops.conv3x3_winograd_bf16
            return {"out": fn(x, u, cout, shift, dilation=d, **kw)}

        def verify(r):
            err = (r["out"].double() - want).abs().max().item()
            if kind == "bf16":
                _lt(err / (1.0 if variant == "head" else max(1.0, ref.abs().max().item())), 2e-2)
            elif variant == "head":
                _lt(err, 1e-5 if kind == "f32" else 2e-5)
            else:
                _lt(err / (1.0 if kind == "f32" else max(1.0, ref.abs().max().item())), 1e-4)
        return run, verify
    return _simple(make)


_WINO = {"f32": ("awseg_conv3x3_winograd_nhwc", "test_gpu_kernels.py::test_conv3x3_winograd_matches_direct (1e-4 abs; head 1e-5)", ()),
         "split": ("awseg_conv3x3_winograd_split_nhwc", "test_gpu_kernels.py::test_conv3x3_winograd_split_float32_grade (1e-4 rel; head 2e-5)",
                   ("awseg_winograd_split_weight_halfs",)),
         "bf16": ("awseg_conv3x3_winograd_bf16_nhwc", "test_gpu_bf16.py::test_conv3x3_winograd_bf16 (2e-2 rel)", ())}
for kind_, (sym_, gate_, sizes_) in _WINO.items():
    for shape_, variant_ in [((1, 33, 35, 16, 64, 1), "plain"), ((2, 16, 32, 16, 64, 1), "residual"), ((1, 40, 72, 16, 64, 2), "residual"),
                             ((1, 33, 35, 16, 64, 1), "head"), ((2, 17, 19, 32, 128, 3), "plain")]:
        add(Case(f"winograd-{kind_}-{'x'.join(map(str, shape_))}-{variant_}", (sym_,), _winograd(kind_, shape_, variant_),
                 "float64 direct conv2d (+ shift, residual, ReLU / 1x1 + sigmoid)", gate_, sizes=sizes_))


# ================================================================================ gathered-operand GEMMs: conv, conv-rows, dual, pieces
def _conv_gemm(cfg):
    def make(device, ops):
        b, h, w, c, n, kh, kw, st, pd = cfg
        g = _gen(device, sum(cfg))
        x = torch.randn(b, h, w, c, device=device, generator=g)
        wt = torch.randn(n, c, kh, kw, device=device, generator=g) * 0.05
        bias = torch.randn(n, device=device, generator=g)
        w2 = wt.permute(0, 2, 3, 1).reshape(n, kh * kw * c).contiguous()
        ref = torch.relu(torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), wt.double(), bias.double(), stride=st, padding=pd))

        def run():
            ws = ops.gemm_split_weights(w2)
            return {"out": ops.conv_gemm_split(x, ws, bias, 1, kh, kw, st, pd), "w_split": ws}
        return run, (lambda r: _lt((r["out"].permute(0, 3, 1, 2).double() - ref).abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item())))
    return _simple(make)


for cfg_ in [(2, 33, 35, 32, 128, 3, 3, 2, 1), (1, 40, 72, 32, 192, 2, 2, 2, 0), (2, 17, 19, 32, 128, 1, 1, 2, 0), (1, 16, 32, 32, 128, 3, 3, 2, 1)]:
    add(Case(f"conv_gemm-{'x'.join(map(str, cfg_))}", ("awseg_conv_gemm_split_bias_act",), _conv_gemm(cfg_), "float64 conv2d + bias, ReLU",
             "test_gpu_kernels.py::test_conv_gemm_split_equals_im2col_plus_gemm (1e-5 of the largest output)", sizes=("awseg_gemm_split_weight_halfs",)))


def _conv_rows(cfg):
    def make(device, ops):
        b, h, w, n = cfg
        g = _gen(device, sum(cfg))
        x = torch.randn(b, 3, h, w, device=device, generator=g) * 2.0
        wt = torch.randn(n, 3, 7, 7, device=device, generator=g) * 0.1
        bias = torch.randn(n, device=device, generator=g)
        wo = (w + 6 - 7) // 2 + 1
        wp = max(w + 3, (wo - 1) * 2 + 8)
        xp = torch.zeros(b, h, wp, 4, device=device)
        xp[:, :, 3:3 + w, :3] = x.permute(0, 2, 3, 1)
        ref = torch.nn.functional.conv2d(x.double(), wt.double(), bias.double(), 2, 3).clamp_min(0).permute(0, 2, 3, 1)

        def run():
            ws = ops.gemm_split_weights(ops.stem_rows_weights(wt))
            return {"out": ops.conv_rows_gemm_split(xp, ws, bias, 1, 7, 2, 3, wo), "w_split": ws}
        return run, (lambda r: _lt((r["out"].double() - ref).abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item())))
    return _simple(make)


# the launcher declines shapes with too few tiles (AWSEG_ERANGE: 1 x 16 x 35 in the family's own test); 3 x 200 x 328 is the smallest shape
# that test pins as accepted, with an odd output width (the last run ends in the right padding)
add(Case("conv_rows-3x200x328x64", ("awseg_conv_rows_gemm_split_bias_act",), _conv_rows((3, 200, 328, 64)), "float64 conv2d 7x7 / 2 + bias, ReLU",
         "test_gpu_kernels.py::test_stem_rows_gemm_matches_conv7x7 (1e-5 of the largest output)", sizes=("awseg_gemm_split_weight_halfs",)))


def _dual(case):
    def make(device, ops):
        mb, k1, k2, n, st = case
        g = _gen(device, sum(case))
        if st == 0:
            m = mb
            x2 = torch.randn(m, k2, device=device, generator=g)
            rows2 = x2
        else:
            x2 = torch.randn(mb, 21, 27, k2, device=device, generator=g)
            rows2 = x2[:, ::st, ::st].reshape(-1, k2)
            m = rows2.shape[0]
        x = torch.randn(m, k1, device=device, generator=g)
        w = torch.randn(n, k1 + k2, device=device, generator=g) / (k1 + k2) ** 0.5
        b = torch.randn(n, device=device, generator=g)
        ref = torch.relu(torch.cat([x, rows2], dim=1).double() @ w.double().t() + b.double())

        def run():
            ws = ops.gemm_split_weights(w)
            return {"out": ops.gemm_split_dual(x, x2, ws, b, 1, stride=st), "w_split": ws}
        return run, (lambda r: _lt((r["out"].double() - ref).abs().max().item(), 2e-5))
    return _simple(make)


for case_ in [(129, 64, 64, 128, 0), (200, 32, 96, 192, 0), (2, 32, 96, 64, 2), (1, 64, 64, 128, 2)]:
    add(Case(f"gemm-dual-{'x'.join(map(str, case_))}", ("awseg_gemm_split_dual_bias_act",), _dual(case_), "float64 relu([x | x2] w^T + b)",
             "test_gpu_kernels.py::test_gemm_split_dual_operand_vs_float64 (2e-5 abs)", sizes=("awseg_gemm_split_weight_halfs",)))


def _pieces(case):
    def make(device, ops):
        m, n, kp, npieces = case
        g = _gen(device, sum(case))
        pieces = [torch.randn(m, kp, device=device, generator=g) for _ in range(npieces)]
        w = torch.randn(n, kp * npieces, device=device, generator=g) / (kp * npieces) ** 0.5
        b = torch.randn(n, device=device, generator=g)
        res = torch.randn(m, n, device=device, generator=g)
        ref = torch.relu(torch.cat(pieces, dim=1).double() @ w.double().t() + b.double() + res.double())

        def run():
            ws = ops.gemm_split_weights(w)
            for p in pieces:
                ops.N.ptr(p)                                        # the pieces travel in a host pointer table: name them to the recorder
            acc = res.clone()
            return {"out": ops.gemm_split_pieces(pieces, ws, b, 1, residual=acc, out=acc), "w_split": ws}
        return run, (lambda r: _lt((r["out"].double() - ref).abs().max().item(), 2e-5))
    return _simple(make)


for case_ in [(129, 128, 64, 2), (200, 192, 32, 4), (300, 512, 128, 2)]:
    add(Case(f"gemm-pieces-{'x'.join(map(str, case_))}", ("awseg_gemm_split_pieces_bias_act",), _pieces(case_),
             "float64 relu(cat(pieces) w^T + b + residual), the residual's buffer is the output",
             "test_gpu_kernels.py::test_gemm_split_pieces_vs_float64 (2e-5 abs)", sizes=("awseg_gemm_split_weight_halfs",)))


# ============================================================================ training step: BatchNorm-ReLU-dropout, depthwise wgrad
def _bn_train(b, c, h, w, p, dx_cl):
    def make(device, ops):
        g = _gen(device, b + c + h + w)
        x0 = torch.randn(b, c, h, w, device=device, generator=g) * 2.0 + 0.5
        gy = torch.randn(b, c, h, w, device=device, generator=g)
        bn0 = torch.nn.BatchNorm2d(c).to(device).train()
        with torch.no_grad():
            bn0.weight.copy_(torch.rand(c, device=device, generator=g) + 0.5)
            bn0.bias.copy_(torch.randn(c, device=device, generator=g) * 0.3)
            bn0.running_mean.copy_(torch.randn(c, device=device, generator=g))
            bn0.running_var.copy_(torch.rand(c, device=device, generator=g) * 1.5 + 0.5)
        state = {k: v.clone() for k, v in bn0.state_dict().items()}
        drop = torch.nn.Dropout2d(p).train() if p > 0 else None

        def run():
            bn = torch.nn.BatchNorm2d(c).to(device).train()
            bn.load_state_dict(state)
            torch.manual_seed(1234)
            xi = x0.clone().requires_grad_(True)
            mid = xi * 1.0                                          # a non-leaf in front keeps the Function's own gradient layout
            seen = []
            mid.register_hook(seen.append)
            y = ops.bn_relu_dropout2d_train(mid, bn, drop, dx_channels_last=dx_cl)
            y.backward(gy)
            return {"out": y.detach(), "dx": seen[0], "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}

        def verify(r):
            ref_bn = torch.nn.BatchNorm2d(c).to(device).double().train()
            ref_bn.load_state_dict(state)
            xd = x0.double().requires_grad_(True)
            torch.manual_seed(1234)
            noise = torch.empty(b, c, 1, 1, device=device).bernoulli_(1.0 - p).div_(1.0 - p).double() if p > 0 else 1.0
            yr = torch.relu(ref_bn(xd)) * noise
            yr.backward(gy.double())
            for name, want in (("out", yr.detach()), ("dx", xd.grad), ("dgamma", ref_bn.weight.grad), ("dbeta", ref_bn.bias.grad)):
                _lt((r[name].double() - want).abs().max().item(), 3e-5 * max(1.0, want.abs().max().item()))
        return run, verify
    return _simple(make)


# one chunk per plane: 4 x 8 (the smallest hw % 4 == 0 plane worth a block); two chunks: 4 x 4097 = launch_geometry.BN_CHUNK + one float4
for cfg_ in [(2, 3, 4, 8, 0.1, False), (2, 3, 4, 4097, 0.1, False), (2, 32, 4, 8, 0.0, True), (2, 32, 4, 4097, 0.1, True)]:
    add(Case(f"bn_train-{'x'.join(map(str, cfg_[:4]))}-p{cfg_[4]}{'-dx-nhwc' if cfg_[5] else ''}",
             ("awseg_bn_train_stats", "awseg_bn_relu_dropout_forward", "awseg_bn_relu_dropout_backward"), _bn_train(*cfg_),
             "float64 nn.BatchNorm2d(train) -> ReLU -> the same Dropout2d draw, autograd",
             "test_gpu_launch_geometry.py::test_bn_relu_dropout2d_train_across_chunks (3e-5 of the largest reference value)",
             sizes=("awseg_bn_train_workspace",)))


def _dw_wgrad(b, h, w, c, d, bias):
    def make(device, ops):
        g = _gen(device, b + h + w + c + d)
        x = torch.randn(b, h, w, c, device=device, generator=g)
        gy = torch.randn(b, h, w, c, device=device, generator=g)
        conv = torch.nn.Conv2d(c, c, 3, 1, d, d, groups=c, bias=bias).to(device).double()
        conv(x.double().permute(0, 3, 1, 2)).backward(gy.double().permute(0, 3, 1, 2))

        def run():
            dw9, db = ops.dwconv3x3_wgrad_nhwc(x, gy, d, want_bias=bias)
            return {"dw9": dw9, "db": db} if bias else {"dw9": dw9}

        def verify(r):
            want = conv.weight.grad.view(c, 9).t()
            _lt((r["dw9"].double() - want).abs().max().item(), 2e-5 * max(1.0, want.abs().max().item()))
            if bias:
                _lt((r["db"].double() - conv.bias.grad).abs().max().item(), 2e-5 * max(1.0, conv.bias.grad.abs().max().item()))
        return run, verify
    return _simple(make)


# one chunk: 9 x 13 pixels; two chunks: 33 x 63 = 2079 pixels > launch_geometry.DW_CHUNK (2048), ragged last chunk
for cfg_ in [(2, 9, 13, 8, 1, True), (1, 33, 63, 4, 1, True), (2, 33, 63, 8, 2, False), (3, 5, 5, 4, 2, True)]:
    add(Case(f"dw_wgrad-{'x'.join(map(str, cfg_[:5]))}", ("awseg_dwconv3x3_wgrad_nhwc",), _dw_wgrad(*cfg_), "float64 torch autograd of the depthwise nn.Conv2d",
             "test_gpu_kernels.py::test_depthwise_conv3x3_train_matches_torch_autograd (2e-5 of the largest reference value)",
             sizes=("awseg_dwconv3x3_wgrad_workspace",)))


# =============================================================================== upsample-free heads, bilinear forms, fused depth head
def _head_inputs(device, b, cmid, h, w, cout, seed):
    g = _gen(device, seed)
    cin = 32
    feat = torch.randn(b, cin, h, w, device=device, generator=g)
    w1 = torch.randn(cmid, cin, 3, 3, device=device, generator=g) / (3.0 * cin ** 0.5)
    scale = torch.rand(cmid, device=device, generator=g) + 0.5
    shift = torch.randn(cmid, device=device, generator=g) * 0.3
    w2 = torch.randn(cout, cmid, device=device, generator=g) / cmid ** 0.5
    b2 = torch.randn(cout, device=device, generator=g)
    g9 = torch.einsum("bchw,ockl->bhwklo", feat, w1 * scale.view(-1, 1, 1, 1)).reshape(b, h, w, 9, cmid).contiguous()   # scale folded
    return feat, w1, scale, shift, w2, b2, g9


def _head_mid64(feat, w1, scale, shift, H, W):
    up = torch.nn.functional.interpolate(feat.double(), size=(H, W), mode="bilinear", align_corners=False)
    return torch.relu(torch.nn.functional.conv2d(up, (w1 * scale.view(-1, 1, 1, 1)).double(), None, padding=1) + shift.double().view(1, -1, 1, 1))


def _seg_head(b, cmid, h, w, H, W, cout, split):
    def make(device, ops):
        feat, w1, scale, shift, w2, b2, g9 = _head_inputs(device, b, cmid, h, w, cout, cmid + H)
        ref = torch.nn.functional.conv2d(_head_mid64(feat, w1, scale, shift, H, W), w2.double().view(cout, cmid, 1, 1), b2.double())
        return (lambda: {"out": ops.segformer_head_fused(g9, None, shift, w2, b2, H, W, split=split)}), \
            (lambda r: _lt((r["out"].double() - ref).abs().max().item(), (1e-5 * ref.abs().max().item()) if split else 1e-4 * max(1.0, ref.abs().max().item())))
    return _simple(make)


_HEAD_GATE = "test_gpu_kernels.py::test_segformer_head_mfma_vs_v1_and_torch (1e-4 of the largest logit); split: test_segformer_head_split_is_float32_grade... (1e-5)"
for cfg_ in [(2, 128, 1, 2, 33, 35, 19), (1, 32, 3, 5, 96, 160, 7), (1, 128, 2, 2, 40, 72, 19), (2, 64, 2, 2, 64, 64, 32)]:
    add(Case(f"segformer_head-{'x'.join(map(str, cfg_))}", ("awseg_segformer_head_fused",), _seg_head(*cfg_, False),
             "float64 conv1x1(relu(bn(conv3x3(interpolate(f)))))", _HEAD_GATE))
for cfg_ in [(2, 128, 1, 2, 33, 35, 19), (1, 128, 2, 2, 40, 72, 19), (1, 256, 5, 7, 160, 224, 19)]:
    add(Case(f"segformer_head-split-{'x'.join(map(str, cfg_))}", ("awseg_segformer_head_fused_split",), _seg_head(*cfg_, True),
             "float64 conv1x1(relu(bn(conv3x3(interpolate(f)))))", _HEAD_GATE))


def _upconv_bn_relu(b, cmid, h, w, H, W, cl):
    def make(device, ops):
        feat, w1, scale, shift, _, _, g9 = _head_inputs(device, b, cmid, h, w, 7, cmid + W)
        ref = _head_mid64(feat, w1, scale, shift, H, W)
        return (lambda: {"out": ops.upconv3x3_bn_relu(g9, None, shift, H, W, channels_last=cl)}), \
            (lambda r: _lt((r["out"].double() - ref).abs().max().item(), 1e-4 * max(1.0, ref.abs().max().item())))
    return _simple(make)


for cfg_ in [(2, 32, 1, 2, 33, 35, False), (1, 64, 2, 2, 40, 72, True), (1, 32, 3, 4, 96, 128, False)]:
    add(Case(f"upconv3x3_bn_relu-{'x'.join(map(str, cfg_[:6]))}{'-nhwc' if cfg_[6] else ''}", ("awseg_upconv3x3_bn_relu",), _upconv_bn_relu(*cfg_),
             "float64 relu(bn(conv3x3(interpolate(f))))", "test_gpu_kernels.py::test_segformer_head_mfma_vs_v1_and_torch (1e-4 of the largest value)"))


def _upconv_train(b, h, w, cin, cmid, H, W):
    def make(device, ops):
        import torch.nn.functional as F
        g = _gen(device, b + h + w + cin + cmid + H + W)
        f = torch.randn(b, cin, h, w, device=device, generator=g)
        wt = torch.randn(cmid, cin, 3, 3, device=device, generator=g) / (3.0 * cin ** 0.5)
        bias = torch.randn(cmid, device=device, generator=g)
        dz = torch.randn(b, cmid, H, W, device=device, generator=g)
        f64, w64, b64 = f.double().requires_grad_(True), wt.double().requires_grad_(True), bias.double().requires_grad_(True)
        ref = F.conv2d(F.interpolate(f64, size=(H, W), mode="bilinear", align_corners=False), w64, b64, padding=1)
        (ref * dz.double()).sum().backward()
        w1r = wt.permute(1, 2, 3, 0).reshape(cin, 9 * cmid).double()

        def run():
            N = ops.N
            g9 = (f.permute(0, 2, 3, 1).reshape(-1, cin) @ w1r.float()).view(b, h, w, 9, cmid).contiguous()
            z = torch.empty(b, cmid, H, W, device=device)
            N.call("awseg_upconv3x3_linear", N.ptr(g9), b, cmid, h, w, H, W, N.ptr(bias), N.ptr(z), 0, N.stream())
            dzl = dz.permute(0, 2, 3, 1).contiguous()
            dg9 = torch.empty(b, h, w, 9, cmid, device=device)
            N.call("awseg_upconv3x3_adjoint", N.ptr(dzl), b, cmid, h, w, H, W, N.ptr(dg9), N.stream())
            return {"z": z, "dg9": dg9}

        def verify(r):
            rel = lambda a, want: (a.double() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)       # noqa: E731
            _lt(rel(r["z"], ref.detach()), 2e-5)
            dtok = (r["dg9"].double().view(-1, 9 * cmid) @ w1r.t()).view(b, h, w, cin).permute(0, 3, 1, 2)
            _lt(rel(dtok, f64.grad), 2e-5)
            _lt(rel(r["dg9"][:, :, :, 4, :].double().sum(dim=(0, 1, 2)), b64.grad), 2e-5)
        return run, verify
    return _simple(make)


for cfg_ in [(2, 1, 2, 16, 32, 33, 70), (1, 2, 2, 16, 32, 64, 64), (1, 3, 4, 16, 32, 100, 130)]:
    add(Case(f"upconv3x3_train-{'x'.join(map(str, cfg_))}", ("awseg_upconv3x3_linear", "awseg_upconv3x3_adjoint"), _upconv_train(*cfg_),
             "float64 torch autograd of conv2d(interpolate(f))", "test_gpu_kernels.py::test_upconv3x3_train_forward_and_adjoint_vs_torch_autograd (2e-5 rel)",
             exact=False, why="awseg_upconv3x3_adjoint accumulates dg9 with float atomicAdd (the launcher zeroes it first)"))


def _depth_fused(b, h, w, cmid, bf16):
    def make(device, ops):
        from tests import forms_ref
        feat, w1, scale, shift, _, _, g9 = _head_inputs(device, b, cmid, h, w, 7, cmid + h + w)
        g = _gen(device, 77)
        wt2 = torch.randn(64, cmid, 3, 3, device=device, generator=g) / (3.0 * cmid ** 0.5)
        shift2 = torch.randn(64, device=device, generator=g) * 0.3
        w2 = torch.randn(64, device=device, generator=g) * 0.2
        b2 = torch.randn(1, device=device, generator=g)
        u = ops.winograd_bf16_weights(wt2) if bf16 else ops.winograd_split_weights(wt2)
        mid = _head_mid64(feat, w1, scale, shift, 32 * h, 32 * w)
        hid = torch.relu(torch.nn.functional.conv2d(mid, wt2.double(), None, padding=1) + shift2.double().view(1, -1, 1, 1))
        ref = torch.sigmoid((hid * w2.double().view(1, -1, 1, 1)).sum(1) + b2.double())

        def run():
            forms = ops.upconv_forms(g9, shift)
            return {"forms": forms, "out": ops.depth_head_fused(forms, h, w, cmid, u, shift2, w2, b2, bf16=bf16)}

        def verify(r):
            forms = _np(r["forms"]).astype(np.float64)
            for i in range(b):
                F4, F2 = forms_ref.build_tables(_np(g9[i]).astype(np.float64), _np(shift).astype(np.float64))
                want = np.concatenate([F4.reshape(-1), F2.reshape(-1)])
                _lt(np.abs(forms[i] - want).max(), 2e-6 * max(1.0, np.abs(want).max()))
            _lt((r["out"].double() - ref).abs().max().item(), 2e-2 if bf16 else 1e-5)
        return run, verify
    return _simple(make)


_DEPTH_GATE = ("test_gpu_kernels.py::test_upconv_forms_table_matches_float64_restatement (2e-6 of the largest entry) / "
               "test_depth_head_fused_matches_as_written_module (1e-5 abs); bf16: test_gpu_bf16.py (2e-2 abs)")
for cfg_ in [(2, 1, 1, 16, False), (1, 1, 2, 32, False), (2, 2, 3, 64, False), (1, 1, 2, 32, True)]:
    add(Case(f"depth_head_fused-{'x'.join(map(str, cfg_[:4]))}{'-bf16' if cfg_[4] else ''}", ("awseg_upconv_forms", "awseg_depth_head_fused"),
             _depth_fused(*cfg_), "tests/forms_ref.py build_tables; float64 as-written depth head on interpolate(f)", _DEPTH_GATE,
             sizes=("awseg_upconv_forms_floats", "awseg_winograd_split_weight_halfs")))


def _mixffn(b, h, w, c):
    def make(device, ops):
        F = torch.nn.functional
        g = _gen(device, b + h + w + c)
        tok = torch.randn(b, h, w, c, device=device, generator=g) * 2.0 + 0.3
        gamma, beta = torch.rand(c, device=device, generator=g) + 0.5, torch.randn(c, device=device, generator=g) * 0.2
        w1, b1 = torch.randn(4 * c, c, device=device, generator=g) / c ** 0.5, torch.randn(4 * c, device=device, generator=g) * 0.1
        wd, bd = torch.randn(4 * c, 1, 3, 3, device=device, generator=g) * 0.3, torch.randn(4 * c, device=device, generator=g) * 0.1
        w2, b2 = torch.randn(c, 4 * c, device=device, generator=g) / (4 * c) ** 0.5, torch.randn(c, device=device, generator=g) * 0.1
        taps = wd.view(4 * c, 9).t().contiguous()
        td = tok.double()
        hid = F.linear(F.layer_norm(td, (c,), gamma.double(), beta.double(), 1e-6), w1.double(), b1.double())
        hid = F.conv2d(hid.permute(0, 3, 1, 2), wd.double(), bd.double(), 1, 1, 1, 4 * c).permute(0, 2, 3, 1)
        ref = td + F.linear(F.gelu(hid), w2.double(), b2.double())
        return (lambda: {"out": ops.mixffn_fused(tok, gamma, beta, 1e-6, w1, b1, taps, bd, w2, b2)}), \
            (lambda r: _lt((r["out"].double() - ref).abs().max().item(), 1e-5 * max(1.0, ref.abs().max().item())))
    return _simple(make)


for cfg_ in [(2, 13, 37, 32), (1, 6, 30, 64), (1, 33, 35, 32), (3, 1, 1, 32)]:
    add(Case(f"mixffn-{'x'.join(map(str, cfg_))}", ("awseg_mixffn_fused",), _mixffn(*cfg_), "float64 tok + fc2(gelu(dwconv(fc1(layer_norm(tok)))))",
             "test_gpu_kernels.py::test_mixffn_fused_matches_float64_ops (1e-5 of the largest output)"))


# ======================================================================== one launch for a batch of mixed conditions (throughput mode)
def _weather_batch(h, w, conds):
    def build(device):
        from adverse_weather_semantic_segmentation_robustness_benchmark_amd.data.preprocessing import WeatherDegradationTransforms
        ops = _ops()
        b = 5
        imgs = np.random.RandomState(b * 1000 + h).randint(0, 255, (b, h, w, 3), dtype=np.uint8)

        def apply(one_launch):
            saved = ops.WEATHER_BATCH
            ops.WEATHER_BATCH = one_launch
            try:
                tf = WeatherDegradationTransforms(seed=None, rng="philox", device=torch.device(device))
                tf._frame_seed = 77
                out = _dev(imgs, device)             # starts as the frames: the caller's copy of a clean frame changes nothing
                norm = torch.empty(b, 3, h, w, device=device)
                tf.apply_batch(_dev(imgs, device), conds, out=out, norm_out=norm, frame_ids=list(range(100, 100 + b)))
            finally:
                ops.WEATHER_BATCH = saved
            return {"out": out, "norm_out": norm}

        def verify(r):
            want = apply(False)                                     # the per-kind launchers on the same draws
            assert torch.equal(r["out"], want["out"]) and torch.equal(r["norm_out"], want["norm_out"])
            assert not np.array_equal(_np(r["out"]), imgs)
        return (lambda: apply(True)), verify
    return build


# the launcher takes width % 4 == 0 and width >= 16 only (AWSEG_ERANGE otherwise): 9 x 13 and 12 x 18 are replaced by 9 x 16 (hw % 16 != 0
# rows of 12 dwords) and 12 x 20; one more row holds a clean frame
_WB_GATE = "test_gpu_kernels.py::test_weather_batch_one_launch_equals_the_per_kind_launchers (bit-exact)"
for h_, w_ in [(9, 16), (12, 20), (16, 32)]:
    add(Case(f"weather_batch-5x{h_}x{w_}", ("awseg_weather_batch",), _weather_batch(h_, w_, ["fog", "night", "rain", "snow", "fog"]),
             "the per-kind launchers on the same Philox draws", _WB_GATE, sizes=("awseg_streak_workspace",)))
# with a clean frame: the launcher writes its norm_out only and leaves the frame's bytes in `out` as they were
add(Case("weather_batch-5x16x32-clean", ("awseg_weather_batch",), _weather_batch(16, 32, ["fog", "night", "rain", "clean", "snow"]),
         "the per-kind launchers on the same Philox draws", _WB_GATE, sizes=("awseg_streak_workspace",), inout=("out",)))


# ============================================= one-pass ensemble statistics and failure counters (the recorded cases of test_gpu_logitscan.py)
def _logit_digest(family, mode, c, tag, lname, with_pred=False):
    """The inputs of the recorded case `name` of tests/test_gpu_logitscan.py (tests/golden/logit_counters.json), the call made on
    pre-filled accumulators; verify takes the fill off again and holds the bytes to the recorded digest."""
    hw, off = {"32x64": (32 * 64, 0), "32x64+1": (32 * 64, 1), "31x53": (31 * 53, 0)}[tag]
    ldt = torch.uint8 if lname == "u8" else torch.int64
    stem = {"evalstats": f"evalstats-m{mode}", "confstats": f"confstats{'-pred' if with_pred else ''}-m{mode}",
            "failure": "failure-single" if mode == 3 else f"failure-ens-m{mode}"}[family]
    name = f"{stem}-C{c}-{tag}-{lname}-x2"

    def build(device):
        import json
        from tests import test_gpu_logitscan as TL
        ops = _ops()
        x = TL._In(4, c, hw, ldt, 2.0, off)
        golden = json.loads(TL.GOLDEN.read_text())[name]
        T = x.T if mode == 0 else None

        def run():
            if family == "failure":
                stats = _prefilled(ops.new_failure_stats(device, TL.SLOTS))
                if mode == 3:
                    ops.failure_stats(x.s1, x.label, stats, x.cond)
                elif mode == 4:
                    ops.ensemble_failure_stats(x.s1, x.s2, 1, None, None, x.label, stats, x.cond, combined=x.s3)
                else:
                    ops.ensemble_failure_stats(x.s1, x.s2, mode, x.w, T, x.label, stats, x.cond)
                return {"stats": stats}
            bins, hist = _prefilled(ops.new_ece_bins(TL.BINS, device, TL.SLOTS)), torch.full((2, TL.HIST), FILL, dtype=torch.int64, device=device)
            if family == "evalstats":
                try:
                    ops.ensemble_eval_stats(x.s1, x.s2, mode, x.w, T, x.label, x.cond, x.edges, bins, hist, -1e-3, 0.70)
                except ops.N.AwsegError:
                    assert "refused" in golden
                return {"bins": bins, "hist": hist}
            counts, oob = _prefilled(ops.new_counts(c, device, TL.SLOTS)), torch.full((1,), FILL, dtype=torch.int64, device=device)
            pred = torch.empty((4, hw), dtype=torch.uint8, device=device) if with_pred else None
            out = {"counts": counts, "oob": oob, "bins": bins, "hist": hist}
            try:
                ops.combine_confusion_stats(x.s1, x.s2, mode, x.w, T, x.label, x.cond, counts, oob, x.edges, bins, hist, -1e-3, 0.70, pred_out=pred)
            except ops.N.AwsegError:
                assert "refused" in golden
            return dict(out, pred=pred) if with_pred else out

        def verify(r):
            if "refused" in golden:                                  # no scalar path: AWSEG_EALIGN then as now, nothing accumulated
                assert "code -3" in golden["refused"] and all(bool((v == FILL).all()) for k, v in r.items() if k != "pred")
                return
            got = TL.digest({k: (v if k == "pred" else v - FILL) for k, v in r.items()})
            assert got["sums"] == golden["sums"] and got["sha256"] == golden["sha256"], name
            if off:
                assert x.s1.data_ptr() % 16 == 4
        return run, verify
    return name, build


_DIGEST_GATE = "test_gpu_logitscan.py::test_counters_are_the_recorded_ones_bit_for_bit (sha256 of the raw bytes)"
_ACC = ("stats", "bins", "ece_bins", "auroc_hist", "counts", "oob")
# the one-pass statistics have vector paths only: 31 x 53 and an off-alignment base are AWSEG_EALIGN (pinned by
# test_off_alignment_and_ragged_frames_are_refused_where_there_is_no_scalar_path), so their rows are the 32 x 64 frames, and the refusals
for lname_ in ("u8", "i64"):
    for mode_ in (0, 2):
        for fam_, sym_, wp_ in (("evalstats", "awseg_ensemble_eval_stats", False), ("confstats", "awseg_combine_confusion_stats", False),
                                ("confstats", "awseg_combine_confusion_stats_pred", True)):
            name_, build_ = _logit_digest(fam_, mode_, 19, "32x64", lname_, wp_)
            add(Case(name_, (sym_,), build_, "tests/golden/logit_counters.json", _DIGEST_GATE, sizes=("awseg_metrics_workspace",), inout=_ACC))
    for tag_ in ("32x64+1", "31x53"):                                # the refusals, as rows: AWSEG_EALIGN, accumulators and pred untouched
        for fam_, sym_, wp_ in (("evalstats", "awseg_ensemble_eval_stats", False), ("confstats", "awseg_combine_confusion_stats", False),
                                ("confstats", "awseg_combine_confusion_stats_pred", True)):
            name_, build_ = _logit_digest(fam_, 0, 19, tag_, lname_, wp_)
            add(Case(name_, (sym_,), build_, "tests/golden/logit_counters.json", _DIGEST_GATE, sizes=("awseg_metrics_workspace",), inout=_ACC,
                     declines={sym_: -3}, partial=("pred",) if wp_ else ()))
    # the failure counters have a scalar path: the same frames one float behind an aligned base, and a ragged frame
    for tag_ in ("32x64", "32x64+1", "31x53"):
        for mode_, sym_ in ((3, "awseg_failure_stats"), (0, "awseg_ensemble_failure_stats"), (2, "awseg_ensemble_failure_stats"),
                            (4, "awseg_ensemble_failure_stats")):
            name_, build_ = _logit_digest("failure", mode_, 19, tag_, lname_)
            add(Case(name_, (sym_,), build_, "tests/golden/logit_counters.json", _DIGEST_GATE, inout=_ACC))
    for mode_, sym_ in ((3, "awseg_failure_stats"), (0, "awseg_ensemble_failure_stats")):
        name_, build_ = _logit_digest("failure", mode_, 7, "31x53", lname_)
        add(Case(name_, (sym_,), build_, "tests/golden/logit_counters.json", _DIGEST_GATE, inout=_ACC))


# ============================================================================================ image-quality and depth-error scanners
def _quality(h, w, maker):
    def build(device):
        from tests import quality_ref as QR
        ops = _ops()
        var, clean, fr, mean, std = getattr(QR, maker)(11 + h + w, 2, 3, h, w)

        def run():
            st = _prefilled(ops.new_image_quality_stats(device, 3))
            oob = torch.full((1,), FILL, dtype=torch.int64, device=device)
            ops.image_quality(_dev(var, device), _dev(clean, device), _dev(np.asarray(fr, np.int32), device), st, cond=_i32(COND, device), oob=oob,
                              mean=mean, std=std)
            return {"stats": st, "oob": oob}

        def verify(r):
            want, bad = QR.counters(var, clean, fr, mean, std, cond=COND, n_slots=3)
            got = _np(r["stats"]) - FILL
            assert np.array_equal(got.reshape(want.shape), want) and r["oob"].item() - FILL == bad
        return run, verify
    return build


for h_, w_ in IMAGE_SHAPES + [(21, 23)]:            # 21 x 23: the smallest ragged frame with more than one row of 11 x 11 windows
    for maker_ in ("rendered_frames", "random_frames"):
        add(Case(f"quality-{maker_.split('_')[0]}-{h_}x{w_}", ("awseg_image_quality",), _quality(h_, w_, maker_), "tests/quality_ref.py counters",
                 "test_gpu_quality.py::test_counters_equal_the_float32_model (bit-exact)", sizes=("awseg_image_quality_workspace",),
                 inout=("stats", "oob")))
for h_, w_ in [(9, 13), (16, 32)]:                  # image and ref_images one float off alignment: the scalar path; 16 x 32 by alignment alone
    add(Case(f"quality-random-{h_}x{w_}-inputs+1", ("awseg_image_quality",), _off_alignment(_quality(h_, w_, "random_frames")),
             "tests/quality_ref.py counters", "test_gpu_quality.py::test_a_base_pointer_off_16_byte_alignment_takes_the_scalar_path (bit-exact)",
             sizes=("awseg_image_quality_workspace",), inout=("stats", "oob"), shifted=("image", "ref_images")))


def _depth_eval(h, w, weighted):
    def build(device):
        from tests import test_gpu_depth_eval as TD
        ops = _ops()
        d1, d2, t = TD.make_inputs(11, 2, h, w)
        wts = torch.softmax(torch.tensor([0.3, 0.7]), 0).numpy() if weighted else None

        def run():
            st = _prefilled(ops.new_depth_eval_stats(device, 3))
            ops.depth_eval_stats(_dev(d1, device), _dev(d2, device), None if wts is None else _dev(wts, device), _dev(t, device), st, 1e-3,
                                 _i32(COND, device))
            return {"stats": st}

        def verify(r):
            TD.check_gate(_np(r["stats"]) - FILL, d1, d2, wts, t, 1e-3, COND, 3, f"fenced {h}x{w}")
        return run, verify
    return build


for (h_, w_), weighted_ in [((9, 13), True), ((12, 18), False), ((16, 32), True), ((37, 53), False)]:
    add(Case(f"depth_eval-{h_}x{w_}-{'weighted' if weighted_ else 'mean'}", ("awseg_depth_eval_stats",), _depth_eval(h_, w_, weighted_),
             "tests/depth_ref.py depth_stats (float64, float32 twin)", "test_gpu_depth_eval.py check_gate (4 x the twin's gap + 2^-21 on the means)",
             inout=("stats",)))


# ================================================================================================= streamed temperature calibration
_TGRID = np.array([0.5, 1.0, 2.5], np.float32)


def _tgrid_inputs(device, c, h, w, ldt, seed, scale=2.0):
    g = _gen(device, seed)
    r = torch.randn(2, c, h, w, device=device, generator=g) * scale
    y = torch.randint(0, c, (2, h, w), device=device, generator=g)
    y[torch.rand(2, h, w, device=device, generator=g) < 0.05] = 255
    return r.contiguous(), y.to(torch.uint8 if ldt == "uint8" else torch.int64).contiguous()


def _tgrid(c, h, w, ldt):
    def make(device, ops):
        import torch.nn.functional as F
        from tests import calib_ref as CR
        from adverse_weather_semantic_segmentation_robustness_benchmark_amd.evaluation.metrics import ConfidenceCalibration
        r, y = _tgrid_inputs(device, c, h, w, ldt, 3)
        edges = torch.linspace(0, 1, 16).to(device)

        def run():
            st = _prefilled(ops.new_temperature_grid_stats(len(_TGRID), 15, device, 3))
            ops.temperature_grid_stats(r, y, st, _TGRID, edges, _i32(COND, device))
            return {"stats": st}

        def verify(res):                                             # the loop of test_grid_nll_and_ece_against_float64, slot 0
            s = ops.temperature_grid_stats_to_numpy(res["stats"] - FILL)
            ref = CR.grid_stats_f64(_np(r), _np(y), _TGRID, _np(edges))
            assert np.array_equal(s["count"][0], ref["count"][0].astype(np.int64)) and not s["nonfinite"].any()
            yl = y.long()
            for k, t in enumerate(_TGRID):
                dev = s["nll_q"][0, k] * CR.NLL_UNIT / s["count"][0, k]
                f64 = ref["nll_sum"][0, k] / ref["count"][0, k]
                per = F.cross_entropy(r / float(t), yl, ignore_index=255, reduction="none")
                twin = per[yl != 255].clamp(max=CR.NLL_CAP).mean().item()
                assert abs(dev - f64) <= CR.nll_gate(abs(twin - f64))
                assert abs(int(s["saturated"][0, k]) - ref["saturated"][0, k]) <= 2
                assert np.abs(s["bins"]["count"][0, k].astype(np.float64) - ref["bin_count"][0, k]).sum() <= 2 * ref["near_edge"][0, k]
                assert abs(ConfidenceCalibration.ece_from_bins(s["bins"][0, k]) - CR.ece_f64(ref, 0, k)) <= 1e-5
            assert np.array_equal(s["count"][0], s["count"][1] + s["count"][2])
        return run, verify
    return _simple(make)


def _tgrid_ensemble(h, w, ldt, mode):
    def make(device, ops):
        s1, y = _tgrid_inputs(device, 19, h, w, ldt, 6, 3.0)
        s2, _ = _tgrid_inputs(device, 19, h, w, ldt, 7, 3.0)
        wts = torch.softmax(torch.tensor([0.3, -0.2], device=device), 0) if mode == 0 else None
        T = torch.tensor([1.3], device=device) if mode == 0 else None
        edges = torch.linspace(0, 1, 16).to(device)

        def run():
            st = _prefilled(ops.new_temperature_grid_stats(len(_TGRID), 15, device, 3))
            ops.ensemble_temperature_grid_stats(s1, s2, mode, wts, T, y, st, _TGRID, edges, _i32(COND, device))
            return {"stats": st}

        def verify(res):                                             # test_t1_ensemble_bins_are_bit_identical_to_the_stats_kernels, last part
            r = (wts[0] * s1 + wts[1] * s2) / T if mode == 0 else (s1 + s2) / 2
            single = _prefilled(ops.new_temperature_grid_stats(len(_TGRID), 15, device, 3))
            ops.temperature_grid_stats(r.contiguous(), y, single, _TGRID, edges, _i32(COND, device))
            assert torch.equal(single, res["stats"])
        return run, verify
    return _simple(make)


for c_ in (7, 19):
    for hw_ in MAP_SHAPES:
        for ldt_ in ("uint8", "int64"):
            add(Case(f"tgrid-{c_}-{hw_[0]}x{hw_[1]}-{ldt_}", ("awseg_temperature_grid_stats",), _tgrid(c_, hw_[0], hw_[1], ldt_),
                     "tests/calib_ref.py grid_stats_f64 (float64) and the float32 torch twin",
                     "test_gpu_calibration.py::test_grid_nll_and_ece_against_float64 (nll_gate of the twin's gap; bins within 2 x near-edge pixels; ECE 1e-5)",
                     inout=("stats",)))
for hw_ in MAP_SHAPES[1:]:                   # C = 19 and hw % 4 == 0 are the entry point's conditions: 5 x 7 has no row
    for ldt_ in ("uint8", "int64"):
        for mode_ in (0, 2):
            add(Case(f"tgrid-ensemble-{hw_[0]}x{hw_[1]}-{ldt_}-mode{mode_}", ("awseg_ensemble_temperature_grid_stats",),
                     _tgrid_ensemble(hw_[0], hw_[1], ldt_, mode_), "awseg_temperature_grid_stats on the materialised combination",
                     "test_gpu_calibration.py::test_t1_ensemble_bins_are_bit_identical_to_the_stats_kernels (bit-exact)", inout=("stats",)))
