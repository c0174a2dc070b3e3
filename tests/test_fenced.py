"""The fence helper on CPU tensors, and the completeness of the case table (no GPU)."""
import re

import pytest
import torch

from tests import fenced
from tests import launch_geometry as G
from tests.fenced_cases import CASES, EXEMPT

PROTOS = fenced.parse_header()


def _arena():
    return fenced.Arena("cpu", fence_bytes=128, capacity=1 << 14)


# ------------------------------------------------------------------------------------------------------------------ the helper
def test_a_byte_in_front_and_a_byte_behind_are_reported_with_their_offsets():
    a = _arena()
    a.take((3, 5), torch.float32, name="x")
    y = a.take(7, torch.uint8, name="y")
    assert a.check() == []
    r = a.region_of(y)
    a.buf[r.start - 1] = 1
    assert a.check() == [("y", "before", -1, 1)]
    a.buf[r.start - 1] = a.fill
    a.buf[r.start + 7] = 2                              # the byte after the last element: nothing is rounded up
    a.buf[r.start + 9] = 2
    assert a.check() == [("y", "after", 7, 2)]
    y.fill_(0)                                          # writing the region itself is no damage
    a.buf[r.start + 7] = a.buf[r.start + 9] = a.fill
    assert a.check() == []


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_poison_refills_fences_outputs_and_scratch_and_keeps_inputs(byte):
    a = _arena()
    x = a.take(5, torch.int64, kind="in", name="x")
    x.copy_(torch.arange(5))
    acc = a.take(3, torch.float64, kind="inout", name="acc")
    acc.fill_(2.5)
    out = a.take((2, 3), torch.float32, kind="out", name="out")
    ws = a.take_bytes(37, name="ws")
    r = a.region_of(out)
    a.buf[r.start + r.nbytes + 3] = 9
    a.poison(byte)
    assert a.check() == []
    assert torch.equal(x, torch.arange(5)) and (acc == 2.5).all()
    assert (out.view(torch.uint8) == byte).all() and (ws == byte).all()
    if byte == 0xFF:
        assert out.isnan().all()
    ws[0] = 1                                           # scratch may be written
    assert a.check() == []


def test_regions_do_not_overlap_offsets_are_honoured_and_workspaces_are_exact():
    a = _arena()
    views = [a.take((3, 5), torch.float32), a.take_bytes(37), a.take(9, torch.uint8, offset_bytes=1),
             a.take(4, torch.float32, offset_bytes=4), a.take_bytes(0), a.take(3, torch.float64, offset_bytes=248)]
    want = [0, 0, 1, 4, 0, 248]
    for v, off in zip(views, want):
        assert v.data_ptr() % 256 == off
    assert views[1].numel() == 37 and a.regions[1].nbytes == 37 and views[4].numel() == 0
    spans = [(r.before, r.start, r.start + r.nbytes, r.after_end) for r in a.regions]
    for (b, s, e, f), n in zip(spans, [60, 37, 9, 16, 0, 24]):
        assert e - s == n and s - b >= a.fence_bytes and f - e == a.fence_bytes
    for prev, cur in zip(spans, spans[1:]):
        assert prev[3] <= cur[0]                        # a region's fences end before the next region's begin
    with pytest.raises(ValueError):
        a.take(2, torch.float32, offset_bytes=2)        # not a multiple of the element
    with pytest.raises(MemoryError):
        a.take_bytes(1 << 14)


def test_unwritten_elements_are_those_that_hold_both_poisons():
    zero = torch.tensor([0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 255, 255, 255, 255], dtype=torch.uint8)
    ones = torch.tensor([255, 255, 255, 255, 1, 0, 0, 0, 0, 0, 0, 0, 255, 255, 255, 255], dtype=torch.uint8)
    assert fenced.unwritten(zero, ones, 4).tolist() == [0]          # 1, 0.0 and NaN were written; element 0 never
    assert fenced.unwritten(zero, ones, 1).tolist() == [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------------------------- completeness
def test_header_parser_sees_every_prototype_and_its_const_qualifiers():
    protos = fenced.parse_header()
    declared = set(re.findall(r"\b(awseg_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", fenced.HEADER.read_text(), flags=re.S)))
    assert declared == set(protos)
    p = {q.name: q for q in protos["awseg_fog_ce_forward"]}
    assert p["logits"].const and p["logits"].pointer and not p["pixel_loss"].const and not p["batch"].pointer
    assert [q.name for q in protos["awseg_bias_act_nhwc"]][:2] == ["x", "n_pixels"] and not protos["awseg_bias_act_nhwc"][0].const
    assert protos["awseg_abi_version"] == []


def unaccounted(protos) -> list:
    return sorted(n for n in protos if not fenced.is_size_function(n) and n not in CASES and n not in EXEMPT)


def test_every_launcher_has_a_case_or_a_stated_exemption(tmp_path):
    protos = fenced.parse_header()
    assert unaccounted(protos) == []
    for table in (CASES, EXEMPT):
        assert set(table) <= set(protos), f"not in the header: {sorted(set(table) - set(protos))}"
    assert not set(CASES) & set(EXEMPT)
    assert all(isinstance(r, str) and r for r in EXEMPT.values())
    # a launcher nobody listed fails
    scratch = tmp_path / "awseg.h"
    scratch.write_text(fenced.HEADER.read_text().replace("#ifdef __cplusplus\n}", "int awseg_new_kernel(const float* x, float* out, "
                                                         "awseg_stream_t stream);\n#ifdef __cplusplus\n}"))
    assert unaccounted(fenced.parse_header(scratch)) == ["awseg_new_kernel"]


def test_every_case_names_launchers_it_is_filed_under_and_its_reference():
    ids = {}
    for name, cases in CASES.items():
        for c in cases:
            assert name in c.launchers and c.reference and c.gate, c.id
            assert c.exact or c.why, f"{c.id}: an inexact row names the atomic that makes it so"
            assert ids.setdefault(c.id, c) is c, f"two cases share the id {c.id}"
            assert all(fenced.is_size_function(s) for s in c.sizes)
            params = {p.name for launcher in c.launchers for p in PROTOS[launcher]}
            assert set(c.offsets) | set(c.partial) | set(c.shifted) <= params, f"{c.id}: offsets / partial name parameters of its launchers"
            assert set(c.declines) <= set(c.launchers)


def test_every_size_function_sizes_a_region_of_some_case():
    protos = fenced.parse_header()
    used = {s for cases in CASES.values() for c in cases for s in c.sizes}
    owed = {s for s in protos if fenced.is_size_function(s)} - used
    assert not owed, f"size functions no case uses: {sorted(owed)}"


def test_the_chunk_seam_rows_are_on_the_side_of_the_seam_they_name():
    """The one-chunk and two-chunk shapes of the loss, BatchNorm and depthwise-wgrad rows, held to tests/launch_geometry.py: a
    constant that moves in the sources moves this model, and a row that has quietly become one-chunk fails here."""
    ids = {c.id for cases in CASES.values() for c in cases}
    for hw, blocks in ((5 * 7, 1), (8 * 16, 1), (13 * 20, 2), (7 * 37, 2)):
        assert G.loss_bpi(hw, 2) == blocks
    assert {"loss-ce-2x19x5x7-uint8", "loss-ce-2x19x8x16-int64", "loss-ce-2x19x13x20-uint8", "loss-ce-2x7x7x37-int64"} <= ids
    assert G.loss_vec(13 * 20) == 4 and G.loss_vec(7 * 37) == 1
    assert G.bn_chunks(4 * 8) == 1 and G.bn_chunks(4 * 4097) == 2 and 4 * 4097 == G.BN_CHUNK + 4
    assert {"bn_train-2x3x4x8-p0.1", "bn_train-2x3x4x4097-p0.1"} <= ids
    assert G.ceil_div(9 * 13, G.DW_CHUNK) == 1 and G.ceil_div(33 * 63, G.DW_CHUNK) == 2 and (33 * 63) % G.DW_CHUNK
    assert {"dw_wgrad-2x9x13x8x1", "dw_wgrad-1x33x63x4x1"} <= ids

