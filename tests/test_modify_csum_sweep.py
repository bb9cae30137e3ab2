"""ingot_gpu_parse_modify / ingot_gpu_parse_modify_csum on the device over
every field, layer, op and `what` (tests/csum_sweep_cases.py): the records equal
the oracle's and the whole arena, the bytes between the frames included,
equals the definition's (oracle rewrite + tests/csum_update_model.py); frames
that a checksum fill sums before and after the rewrite also equal rewrite +
fill.  Layouts: indexed frames at odd addresses (k_parse), fixed slots on the
ring kernel (k_modify_pipe) and the same slots with pipe = 1 (k_parse).
tests/test_csum_sweep_model.py holds the expected values to a second way of
computing them on the CPU.  Needs an MI355X: `pytest -m gpu`."""
import pytest

import ingot_amd
from ingot_amd import Chain, Field
from ingot_amd.abi import TUNE_PIPELINE
from tests import csum_sweep_cases as sc
from tests.test_modify_csum import on_gpu, same

pytestmark = pytest.mark.gpu
TUN = sc.TUN
chains = pytest.mark.parametrize("chain", sc.CHAINS, ids=lambda c: c.name)


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def kernels(torch):
    """layout -> the contexts that run it: slots go to the ring kernel by
    default and to k_parse with pipe = 1 (the tunnel: k_parse either way)."""
    ring, pipe1 = ingot_amd.Context(0), ingot_amd.Context(0)
    pipe1.set_tuning(TUNE_PIPELINE, 1)
    return {"indexed": (("k_parse", ring),),
            "strided": (("ring", ring), ("pipe=1", pipe1))}


def _contexts(kernels, chain, layout):
    return kernels[layout][:1] if chain == TUN else kernels[layout]


def _run_case(torch, kernels, chain, layout, b, edits, what, two_pass=True, label=None):
    """One edit list under one `what` (0: the plain rewrite) on every kernel
    of the layout.  -> the frames the rewrite changed."""
    want, rewritten, recs, ch = sc.define(b, chain, edits, what)
    tp = both = None
    if what and two_pass and ch.size:
        q = sc.qualifies(b, chain, edits, rewritten, recs, ch)
        both = ch[q[ch]]
        if both.size:
            tp = sc.two_pass(b, chain, rewritten, recs, ch, what)
    for kname, c in _contexts(kernels, chain, layout):
        t = sc.tag(chain, f"{label or layout}/{kname}", edits, what)
        got, g_rec = on_gpu(torch, c, b.arena, b.off, b.lens, chain, edits, what, stride=b.stride,
                            n=b.n)
        assert g_rec.tobytes() == recs.tobytes(), t
        same(got, want, t)
        if tp is not None:
            bad = sc.frames_differ(b, got, tp, both)
            assert bad is None, (t, "two-pass", bad)
    return ch


def _whats(chain, layout, field=None):
    """0 = the plain rewrite.  The five fields the fused update refuses run
    plain only; the tunnel's slots (the indexed frames again, padded) take the
    plain rewrite and all three sums."""
    if field is not None and field in sc.REFUSED:
        return (0,)
    if chain == TUN and layout == "strided":
        return (0, 7)
    return (0,) + sc.WHATS[chain]


@pytest.mark.parametrize("field", list(Field), ids=lambda f: f.name)
@chains
def test_single_edit_sweep(torch, kernels, chain, field):
    moved = 0
    for layout in ("indexed", "strided"):
        b = sc.batch(chain, layout)
        for e in sc.sweep(chain, field):
            for what in _whats(chain, layout, field):
                # the two-pass comparison: every `what` (the tunnel: all sums)
                ch = _run_case(torch, kernels, chain, layout, b, [e], what,
                               two_pass=chain != TUN or what == 7)
                moved += int(ch.size > 0)
    assert (moved > 0) == (field in sc.fields_of(chain)), moved


def test_refused_fields_are_refused(torch, kernels):
    b = sc.batch(Chain.GenericUlp, "indexed")
    c = kernels["indexed"][0][1]
    for f in sc.REFUSED:
        with pytest.raises(RuntimeError, match="parse_modify_csum"):
            on_gpu(torch, c, b.arena, b.off, b.lens, Chain.GenericUlp, [(1, f, sc.SET, 5)], 3)


@chains
def test_dependent_lists(torch, kernels, chain):
    for layout in ("indexed", "strided"):
        for name, edits, prepared in sc.dependent_lists(chain):
            b = sc.batch(chain, layout, prepared)
            zero = ones = udp = ()
            if prepared:
                b, zero, ones, udp = sc.other_repr(b, chain)
            for what in _whats(chain, layout):
                # (the prepared batches hold sums in the representation fill
                # does not write: the definition only)
                _run_case(torch, kernels, chain, layout, b, edits, what,
                          two_pass=not prepared and (chain != TUN or what == 7))
                if not name.startswith("inverse"):
                    continue
                # an edit and its inverse: every byte, the checksum fields in
                # either representation of a zero sum included, is untouched
                for kname, c in _contexts(kernels, chain, layout):
                    got, _ = on_gpu(torch, c, b.arena, b.off, b.lens, chain, edits, what,
                                    stride=b.stride, n=b.n)
                    t = (name, sc.tag(chain, f"{layout}/{kname}", edits, what))
                    assert all(got[a] == 0 and got[a + 1] == 0 for a in zero), t
                    assert all(got[a] == 0xFF and got[a + 1] == 0xFF for a in ones), t
                    assert all(got[a] == 0xFF and got[a + 1] == 0xFF for a in udp), t
                    assert got.tobytes() == b.arena.tobytes(), t


@chains
def test_second_edit_of_a_field_across_the_window(torch, kernels, chain):
    """Every frame at each of the 16 places in its 16-B block: the staged
    window then ends inside every field it can, and the second edit of such a
    field must read the first edit's bytes from both sides of that end (the
    staged copy before it, HBM past it).  Plain rewrite and all sums."""
    lists = [(n, e) for n, e, _ in sc.dependent_lists(chain)
             if n in ("twice across the window", "twice sub sub", "twice set add", "16 nat",
                      "8 to all-ones and back")]
    assert len(lists) == 5
    for mis in range(16):
        b = sc.batch_at(chain, mis)
        assert (b.off % 16 == mis).all()
        for name, edits in lists:
            for what in (0, sc.WHATS[chain][-1]):
                _run_case(torch, kernels, chain, "indexed", b, edits, what, two_pass=False,
                          label=f"indexed at {mis} mod 16")


@chains
def test_random_lists(torch, kernels, chain):
    """200 seeded lists of 1-16 edits, the `what` values in turn, against the
    definition (whole arena); the tunnel on its indexed frames."""
    lists = sc.random_lists(chain)
    assert len(lists) == 200 and max(len(e) for e in lists) == 16
    touched = 0
    for layout in ("indexed",) if chain == TUN else ("indexed", "strided"):
        b = sc.batch(chain, layout)
        for k, edits in enumerate(lists):
            what = sc.WHATS[chain][k % len(sc.WHATS[chain])]
            ch = _run_case(torch, kernels, chain, layout, b, edits, what, two_pass=False)
            touched += int(ch.size > 0)
    assert touched >= 150, touched
