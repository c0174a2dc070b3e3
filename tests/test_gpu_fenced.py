"""-m gpu: what every launcher does OUTSIDE the buffers it was given, and what it assumes about bytes it never wrote.

Each row of tests/fenced_cases.py is one call pattern of the package's ops.  It runs three times on the same input values:

  1. plain    ordinary torch buffers; the result is held to the family's float64 / oracle reference under the family's existing
              gate (so a wrong baseline cannot bless the other two), and the launches are recorded (tests/fenced.py);
  2. fenced   the recorded launches with every device pointer moved into one arena: 64 KiB of fence on both sides of every
              buffer, workspaces of exactly the size function's bytes, fences + outputs + workspaces poisoned with 0x00;
  3. fenced   the same with 0xFF (NaN as a float, -1 as an integer, 255 as a label);
  4. fenced   the same with 0x7F (3.4e38 as a float, a large positive integer: what a maximum folded over a workspace that was
              never cleared would keep, where the -1 of run 3 loses against every real value).

Asserted: no fence byte changed; outputs and accumulators of runs 2 to 4 equal run 1 bit for bit (rows marked exact = False pass
the family's gate instead); no output element still holds its poison in both runs; inputs are unchanged; and the same launches
once more on the workspace the last run left dirty give the same result again.  A difference between the fenced runs means the
result depends on bytes the kernel does not own: a read past an input, or an assumption about what a workspace holds.
"""
import pytest
import torch

from tests import fenced
from tests.fenced_cases import CASES

pytestmark = pytest.mark.gpu

ALL = [c for cases in CASES.values() for c in cases]
UNIQUE = list({c.id: c for c in ALL}.values())
PROTOS = fenced.parse_header()
UNIT = {"_workspace": 1, "_halfs": 2, "_floats": 4, "_partials": 8}


def _plain(case):
    run, verify = case.build("cuda")
    trace = fenced.Trace()
    with fenced.record(trace):
        results = run()
    torch.cuda.synchronize()
    return trace, results, verify


def _differing(a: dict, b: dict) -> list:
    return [k for k in a if not torch.equal(a[k].contiguous().view(-1).view(torch.uint8), b[k].contiguous().view(-1).view(torch.uint8))]


def _compare(case, replay, results, verify, what):
    if case.exact:
        for s in replay.slots:
            if s.kind in ("out", "inout") and s.params.isdisjoint(case.partial):
                diff = (s.region.view != s.final).nonzero()
                assert diff.numel() == 0, (f"{case.id}, {what}: {s.region.name} differs from the plain run in {diff.numel()} bytes, "
                                           f"first at byte {int(diff[0])} of {s.nbytes}")
    else:
        verify({k: replay.view_like(v) for k, v in results.items()})


@pytest.mark.parametrize("case", UNIQUE, ids=[c.id for c in UNIQUE])
def test_fenced(native, case):
    trace, results, verify = _plain(case)
    assert results, "a case names the tensors it defines"
    verify(results)                                                       # run 1 against the family's reference, existing gate
    launched = {l.name for l in trace.launches}
    assert set(case.launchers) <= launched, f"{case.id} did not reach {set(case.launchers) - launched}"
    declined = {l.name: l.rc for l in trace.launches if l.rc != 0}
    assert declined == dict(case.declines), f"{case.id}: launchers declined {declined}, the table says {dict(case.declines)}"

    # exact or not is observed, not assumed: the same call on fresh ordinary buffers
    _, again, _ = _plain(case)
    differing = [k for k in _differing(results, again) if k not in case.partial]
    if case.exact:
        assert not differing, f"{case.id} is marked exact but two plain runs differ in {differing}"

    # every workspace is exactly what its size function said
    slots = fenced.plan(trace, PROTOS, inout=case.inout, scratch=case.scratch)
    called = {n: r for n, _, r in trace.sizes}
    for fn in case.sizes:
        assert fn in called, f"{case.id} names {fn} but the call pattern never asked it"
        unit = next(u for suf, u in UNIT.items() if fn.endswith(suf))
        want = {r * unit for n, _, r in trace.sizes if n == fn}
        have = {b.nbytes for b in trace.buffers.values()} | {s.nbytes for s in slots}
        if fn == "awseg_winograd_split_weight_halfs":
            want = {w + 16 for w in want}                                 # the image, then 2^eu as one float32 in a 16-byte trailer (awseg.h)
        if fn.endswith("_floats"):
            want = {w * n for w in want for n in range(1, 5)}             # awseg_upconv_forms_floats is per frame
        assert want & have, f"{case.id}: no buffer of exactly {fn}'s {sorted(want)} bytes (buffers: {sorted(have)})"
    for b in trace.buffers.values():
        if b.requested is not None and not case.free_workspace:
            assert b.requested in {r * u for n, _, r in trace.sizes for u in (1, 8)}, \
                f"{case.id}: a workspace of {b.requested} bytes that no size function returned"

    for name in case.shifted:                                             # the row says these inputs sit off alignment: they do
        addrs = [fenced._addr(a) for l in trace.launches for p, a in zip(PROTOS[l.name], l.args) if p.name == name]
        assert addrs and all(a % 16 for a in addrs), f"{case.id}: {name} is 16-byte aligned"

    replay = fenced.Replay(trace, slots, "cuda", fence_bytes=case.fence_bytes, offsets=case.offsets, protos=PROTOS)
    after = {}
    for byte in (0x00, 0xFF, 0x7F):
        replay.run(byte)
        damage = replay.arena.check()
        assert not damage, f"{case.id}, poison {byte:#04x}: bytes outside a region changed: {damage}"
        for s in slots:
            if s.kind == "in":
                assert torch.equal(s.region.view, s.initial), f"{case.id}: input {s.region.name} was modified"
        _compare(case, replay, results, verify, f"poison {byte:#04x}")
        after[byte] = {id(s): s.region.view.clone() for s in slots if s.kind == "out"}
        if case.declines:                                                 # a launcher that declined wrote nothing
            for s in slots:
                if s.kind == "out" and not s.params.isdisjoint(case.partial):
                    assert bool((s.region.view == byte).all()), f"{case.id}: {s.region.name} was written by a call that declined"
    for s in slots:
        if s.kind == "out" and s.params.isdisjoint(case.partial):
            left = fenced.unwritten(after[0x00][id(s)], after[0xFF][id(s)], s.elem)
            assert left.numel() == 0, f"{case.id}: {left.numel()} elements of {s.region.name} were never written, first {int(left[0])}"

    if any(s.kind == "scratch" for s in slots):                            # a ticket or counter that does not reset itself
        replay.load()
        replay.launch()
        assert not replay.arena.check()
        _compare(case, replay, results, verify, "second call on the dirty workspace")
