"""No GPU: every case table of tests/test_gpu_launch_geometry.py crosses what it claims, by the launch rules restated in
tests/launch_geometry.py from the constants of the HIP sources.  An entry edited to a shape that stays inside one chunk / one trip /
one span fails here."""
import numpy as np

from tests import launch_geometry as G
from tests import test_gpu_launch_geometry as T


def test_constants_are_the_sources():
    assert G.BN_CHUNK == 16384 and G.BN_T == 256 and G.DW_CHUNK == 2048
    assert G.AWSEG_CUS == 256 and G.MAX_BLOCKS == 2048 == G.LOSS_CAP
    assert G.LOSS_THREADS == G.BACKBONE_THREADS == G.HEADS_THREADS == G.SMALLOPS_THREADS == 256
    assert G.STEM_SPAN == 256 and G.DEPTH_UP_CAP == 1024


def test_rules_on_known_points():
    assert G.grid_1d(0, 256) == 1 and G.grid_1d(257, 256) == 2 and G.grid_1d(10 ** 9, 256) == 2048 and G.grid_1d(10 ** 9, 256, 1024) == 1024
    assert [G.bn_chunks(v) for v in (4, 16384, 16388, 32768, 32772)] == [1, 1, 2, 2, 3]
    assert G.loss_bpi(100, 1) == 1 and G.loss_bpi(1024 * 2048, 2) == 1024 and G.loss_bpi(1540, 2048) == 1 and G.loss_bpi(8000, 300) == 7
    assert G.stride_loop(385, 256, 1) == {"blocks": 1, "trips": 2, "tail": 129, "ragged": True}
    assert G.stride_loop(512, 256, 1)["ragged"] is False
    assert [G.layernorm_lanes(c) for c in (32, 64, 128, 160, 256, 320, 512, 1024)] == [8, 16, 32, 64, 64, 32, 32, 64]
    # the existing unit shapes stay inside one chunk / one trip / one span: the gap this file's GPU half closes
    assert all(G.bn_chunks(hw) == 1 for hw in (60, 2048, 16, 8580))
    assert all(G.layernorm_loop(r, c)["trips"] == 1 for r, c in ((1000, 32), (257, 64), (130, 160), (64, 256), (33, 320), (20, 512), (7, 1024)))
    assert all(G.stem_spans(w)[0] == 1 for w in (37, 64, 16))
    assert G.loss_loop(1024 * 2048, 2)["trips"] == 2


def test_bn_cases_cross_their_chunks():
    for B, C, H, W, p, chunks, last_block in T.BN_CASES:
        hw = H * W
        assert hw % 4 == 0 and G.bn_chunks(hw) == chunks, (H, W)
        if last_block is not None:
            assert C % 32 == 0 and G.bn_nhwc_blocks(hw)[1] == last_block and last_block % 256 != 0
    planes = [c[2] * c[3] for c in T.BN_CASES]
    assert G.BN_CHUNK in planes and G.BN_CHUNK + 4 in planes                         # one full chunk; the second chunk is one float4
    three = [c for c in T.BN_CASES if c[5] >= 3]
    assert any(c[0] > 2 and c[1] > 1 and (c[2] * c[3]) % G.BN_CHUNK for c in three)      # b, c, chunk above 0 and a ragged last chunk
    assert sum(c[6] is not None for c in T.BN_CASES) == 2 and {c[5] for c in T.BN_CASES if c[6] is not None} == {2, 3}
    assert any(c[1] // 32 >= 2 for c in T.BN_CASES if c[6] is not None)               # two 32-channel slices


def test_loss_cases_take_a_second_trip_in_every_instance():
    for name, B, C, H, W, ldt, dens, instance, blocks, trips, tail in T.LOSS_CASES:
        hw = H * W
        loop = G.loss_loop(hw, B)
        assert G.loss_instance(hw, C) == instance, name
        assert (loop["blocks"], loop["trips"], loop["tail"]) == (blocks, trips, tail) and trips >= 2 and loop["ragged"], (name, loop)
        assert hw // G.loss_vec(hw) > blocks * G.LOSS_THREADS
    assert {c[7] for c in T.LOSS_CASES} == {"vec4_ct19", "vec4_ct0", "vec1_ct0"}
    mid = [c for c in T.LOSS_CASES if c[8] > 1]
    assert mid and all(c[10] < c[8] * G.LOSS_THREADS - G.LOSS_THREADS for c in mid)     # some blocks of an image take one trip fewer
    # test_loss_vs_oracle's shapes are one trip: they are here for the normalised gradient gate alone
    assert all(G.loss_loop(s[2] * s[3], s[0])["trips"] == 1 for s in T.LOSS_ORACLE_SHAPES)


def test_density_cases_take_a_second_trip_and_their_reference_is_decided():
    for B, H, W, seed, blocks, trips, tail in T.DENSITY_CASES:
        loop = G.loss_loop(H * W, B, vec=1)
        assert (loop["blocks"], loop["trips"], loop["tail"]) == (blocks, trips, tail) and trips >= 2 and loop["ragged"]
        depth = G.density_depth_input(B, H, W, seed)
        ref, kept = G.density_from_depth_ref(depth, T.DENSITY_MARGIN)
        assert ref.shape == depth.shape and ref.min() >= 0.0 and ref.max() <= 1.0
        assert 1.0 - kept.mean() <= T.DENSITY_MAX_LEFT_OUT
        assert 0.2 < (ref < 0.7 * (depth - depth.min()) / (depth.max() - depth.min()) - 0.1).mean() < 0.8      # the threshold splits the pixels
    assert max(c[0] * c[4] for c in T.DENSITY_CASES) >= 2048                                     # partials for the one-wave finish


def test_density_reference_on_a_hand_example():
    d = np.array([[[0.0, 1.0, 3.0], [0.0, 0.0, 0.0]]], np.float32)
    ref, kept = G.density_from_depth_ref(d)
    gx = np.array([[1.0, 2.0, 2.0], [0.0, 0.0, 0.0]])
    gy = np.array([[0.0, 1.0, 3.0], [0.0, 1.0, 3.0]])
    mag = np.sqrt(gx ** 2 + gy ** 2 + 1e-8)
    want = np.clip(d[0] / (3.0 + 1e-8) * 0.7 - 0.3 * (mag > mag.mean()), 0.0, 1.0)
    assert np.allclose(ref[0], want, atol=1e-15) and kept.all()


def test_stem_cases_cross_their_spans():
    assert T.STEM_B * T.STEM_H > 1
    for W, spans, last in T.STEM_CASES:
        assert G.stem_spans(W) == (spans, last)
    assert [c[1] for c in T.STEM_CASES] == [1, 2, 2, 3] and max(c[1] for c in T.STEM_CASES) >= 3
    assert T.STEM_CASES[0][2] == G.STEM_SPAN and all(c[2] % G.WAVE for c in T.STEM_CASES[1:])     # one full span; ragged last spans


def test_layernorm_cases_take_a_second_trip_in_every_instance():
    for rows, C, lanes in T.LAYERNORM_CASES:
        loop = G.layernorm_loop(rows, C)
        assert G.layernorm_lanes(C) == lanes and loop["blocks"] == G.MAX_BLOCKS and loop["trips"] == 2 and loop["ragged"], (rows, C, loop)
    assert sorted({c[2] for c in T.LAYERNORM_CASES}) == [8, 16, 32, 64]
    by_c = {c[1]: c[2] for c in T.LAYERNORM_CASES}
    assert (320 // 4) / by_c[320] == 2.5 and 160 // 4 == 40 < by_c[160] and (1024 // 4) // by_c[1024] == 4


def test_rowdot_cases_cover_short_ragged_and_full_steps():
    step = 16 * 4
    assert all(k % 4 == 0 for k in T.ROWDOT_K)
    assert min(T.ROWDOT_K) == 4 and any(k < step and k % step for k in T.ROWDOT_K) and step in T.ROWDOT_K
    assert any(k > step and k % step for k in T.ROWDOT_K) and any(k >= 2 * step and k % step == 0 for k in T.ROWDOT_K)
    assert 1 in T.ROWDOT_ROWS and any(r % 16 for r in T.ROWDOT_ROWS) and max(T.ROWDOT_ROWS) * 16 > G.SMALLOPS_THREADS


def _crosses(items, per_block=256, cap=None):
    loop = G.capped_1d(items, per_block, cap)
    return loop["trips"] >= 2 and loop["ragged"] and items < 1.05 * loop["blocks"] * per_block


def test_audit_cases_cross_the_grid_cap_and_the_existing_ones_are_as_the_audit_says():
    B, H, W, C = T.AUDIT_BIAS_ACT
    assert _crosses(G.items_bias_act(B * H * W, C))
    assert _crosses(G.items_im2col(*T.AUDIT_IM2COL))
    assert _crosses(G.items_maxpool(*T.AUDIT_MAXPOOL))
    for kernel, (B, H, W, C, d) in T.AUDIT_DWCONV.items():
        got, items = G.items_dwconv(B, H, W, C, d)
        assert got == kernel and _crosses(items), (kernel, items)
    assert T.AUDIT_UPCAT[3] // 4 % G.UP_QUADS and _crosses(G.items_upcat(*T.AUDIT_UPCAT))
    B, C, h, w, H, W = T.AUDIT_UPSAMPLE_ROWS
    for align in (False, True):
        kernel, items = G.items_upsample(B * C, h, w, H, W, align)
        assert kernel == "rows" and _crosses(items)
    B, h, w, C = T.AUDIT_ASPP
    assert G.aspp_kernel(w, C) == "flat" and _crosses(G.items_aspp(B, h, w, C))
    B, C, H, W = T.AUDIT_STEM
    stem = G.capped_1d(B * H * G.stem_spans(W)[0], G.SMALLOPS_THREADS // G.WAVE)          # a wave per span
    assert stem["trips"] == 2 and stem["tail"] % (G.SMALLOPS_THREADS // G.WAVE) and G.stem_spans(W)[0] >= 3
    # the rows of the audit in the GPU file's docstring: item counts of the largest existing unit cases
    cap = G.MAX_BLOCKS * 256
    assert G.items_bias_act(1 * 32 * 64, 64) == 32768 < cap
    assert max(G.items_im2col(*c[:8], k_padded=(c[4] * c[5] * c[3] + 7) // 8 * 8) for c in (
        (2, 17, 23, 8, 3, 3, 2, 1), (1, 32, 64, 32, 8, 8, 8, 0), (2, 16, 20, 160, 2, 2, 2, 0), (1, 9, 11, 4, 3, 3, 2, 1), (2, 12, 16, 128, 3, 3, 2, 1))) == 27648
    assert max(G.items_maxpool(*s) for s in ((2, 17, 23, 8), (1, 64, 128, 64), (3, 9, 10, 4), (1, 1, 7, 12))) == 16384
    dw = [G.items_dwconv(*c) for c in ((2, 9, 13, 8, 1), (1, 33, 47, 128, 1), (2, 20, 24, 64, 12), (1, 64, 96, 304, 1), (3, 5, 5, 4, 2), (2, 17, 23, 24, 1),
                                       (2, 17, 23, 24, 3))]
    assert max(n for k, n in dw if k == "strip2") == 29184 and max(n for k, n in dw if k == "plain") == 15360 and not [n for k, n in dw if k == "strip"]
    assert max(G.items_upcat(*s) for s in ((2, 5, 7, 8, 4), (1, 16, 32, 256, 48), (1, 3, 3, 4, 4), (2, 9, 13, 256, 8), (1, 4, 21, 512, 48))) == 12288
    up = [G.items_upsample(c[0] * c[1], *c[2:]) for c in ((2, 19, 16, 32, 64, 128, True), (1, 3, 7, 5, 28, 20, True), (2, 1, 4, 8, 64, 128, False),
                                                           (1, 2, 5, 9, 33, 70, False), (1, 19, 256, 512, 1024, 2048, True), (2, 4, 8, 8, 16, 16, False),
                                                           (1, 2, 9, 12, 18, 24, True), (1, 1, 6, 6, 5, 4, True))]
    assert max(n for k, n in up if k == "4x4") == 2490368 > cap and max(n for k, n in up if k == "rows") == 1188
    assert G.aspp_kernel(28, 16) == "flat" and G.items_aspp(2, 20, 28, 16) == 4480
    assert all(G.aspp_kernel(w, c) != "flat" for w, c in ((52, 128), (20, 64), (7, 64), (75, 192)))
    assert G.depth_up_loop(1024, 2048)["trips"] == 8 and 1024 * 2048 > G.DEPTH_UP_CAP * 256
    assert 2 * 9 * G.stem_spans(37)[0] == 18 < G.MAX_BLOCKS * 4
