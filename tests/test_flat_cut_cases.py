"""The conditions the inputs of test_gpu_flat_cut.py are built to hold (flat_cut_cases.py), checked
on the CPU: the coverage of (length, start mod 16) pairs per layout and form, the crafted sums and
the places of their completing words, the two layouts of family C, and that the expectations tell
five deliberately wrong models of the checksum from the right one."""
import numpy as np
import pytest

import flat_cut_cases as X

ALL = {(l, s) for l in X.LENGTHS for s in range(16)}
SUBSET = {(l, s) for l in X.DENSE for s in range(16)} | {(l, s) for l in X.EDGE for s in X.FEW}


def test_lengths_straddle_every_threshold():
    assert X.DENSE == list(range(273))
    for t in X.THRESHOLDS:
        assert set(range(t - 17, t + 18)) <= set(X.EDGE)
    assert set(range(65502, 65536)) <= set(X.EDGE) and max(X.LENGTHS) == 65535
    # the thresholds the issue names are all there; the dispatch code adds kSegTabMax * 16
    assert {384, 768, 1024, 1536, 3072, 6144, 8192, 12288, 32768} <= set(X.THRESHOLDS)
    assert {63, 64, 65, 191, 192, 193} <= set(X.DENSE) and set(X.LARGE_LENGTHS) <= set(X.LENGTHS)


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_default_form_holds_every_pair(layout):
    have = X.plan(layout, "A", True).pairs()
    missing = ALL - have - set(X.EXEMPT[layout])
    assert not missing, sorted(missing)[:8]
    assert not X.EXEMPT[layout]                      # every exclusion is listed with its reason: there is none


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_other_forms_hold_dense_and_edge_starts(layout):
    missing = SUBSET - X.plan(layout, "A", False).pairs()
    assert not missing, sorted(missing)[:8]


def test_forms_name_every_tunable_value():
    values = {k: set() for k in X.DEFAULTS}
    for tunables, _ in X.FORMS.values():
        for k in X.DEFAULTS:
            values[k].add(tunables.get(k, X.DEFAULTS[k]))
    assert values["gather"] >= {1, 0, -1} and values["short_loads"] >= {-1, 0, 1, 2, 3}
    assert values["stream"] >= {-1, 2, 4, 8, 0} and values["chunk_packets"] >= {0, 1, 2, 16, 64}
    assert any(jw for _, jw in X.FORMS.values()) and X.FORMS["default"] == ({}, False)
    assert {4, 8, 32} <= values["chunk_packets"]            # the chunk sizes only the default dispatch picked


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_large_form_holds_the_subset_but_its_listed_exclusions(layout):
    """chunk_packets 0 on a large batch: all of DENSE at 16 starts and EDGE at starts 0, 1, 8, 15,
    but for the lengths LARGE_EXEMPT lists with their reasons."""
    exempt = X.LARGE_EXEMPT[layout]
    assert all(isinstance(r, str) and len(r) > 40 for r in exempt.values())
    want = {(l, s) for l, s in SUBSET if l not in exempt}
    if layout == "odd":
        assert not want and "cp8" in X.FORMS
        return
    if layout in ("b2b", "gap16"):
        bands = X.large_strided(layout)
        have = {(l, b) for _, calls in bands for l, bases in calls for b in bases}
        assert len(bands) == 1 + len(X.THRESHOLDS) and max(l for l, _ in have) < 40000
    else:
        plan = X.cached((layout, "large"), lambda: X.large_plan(layout))
        assert all(c.n >= X.LARGE_N for c in plan.calls)
        have = plan.pairs()
    assert have >= want, sorted(want - have)[:8]
    assert set(X.DENSE) <= {l for l, _ in want}


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_layout_shapes(layout):
    """Outputs at even and odd element offsets with odd and even counts; odd strides with n >= 67;
    CSR: an odd first offset and empty packets at the front, in the middle and at the end; ring
    slots: a length equal to the stride in every call, an odd stride, strides 2048 and 65536."""
    p = X.plan(layout, "A", True)
    if True:
        assert {(int(pos) & 1, c.n & 1) for c, pos in zip(p.calls, p.out_pos)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if layout == "odd":
        assert all(c.stride % 16 == 1 and c.n >= 67 and c.n % 16 and c.stride > c.length for c in p.calls)
    if layout == "gap16":
        assert all(c.stride % 16 == 0 and c.stride > c.length for c in p.calls)
    if layout in ("csr", "seeded"):
        c = p.calls[0]
        ln = c.plen
        assert c.offsets[0] & 1 and not ln[:3].any() and not ln[-4:].any()
        mid = np.flatnonzero(ln[3:-4] == 0)
        assert any((ln[3 + m:3 + m + 5] == 0).all() for m in mid)
    if layout == "seeded":
        assert set(X.SEED_STATES) < set(p.calls[0].states.tolist())
    if layout == "slotted":
        assert {c.stride for c in p.calls} == {2048, 65536, 273, 1584}
        assert all(int(c.lens[-1]) == min(c.stride, 65535) for c in p.calls)
        buf, base, stride, lens = X.clamp_case()
        assert np.count_nonzero(lens > stride) == 1


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_crafted_sums_and_their_completing_words(oracle, layout):
    plan, marks = X.cached((layout, "B"), lambda: X.plan_b(layout))
    seen = set()
    crafted = zeros = 0
    for k, i, p in marks:
        c = plan.calls[k]
        buf, start, length = plan.bufs[c.buf], int(c.start[i]), int(c.plen[i])
        got = oracle.inverted(buf, start, length)
        if p is None:
            assert got == 0 and not buf[start:start + length].any()
            zeros += 1
        else:
            assert got == 0xFFFF and X.word_sum(buf[start:start + length]) % 0xFFFF == 0
            seen |= X.position_tags(length, start, p)
            crafted += 1
    assert seen == set(X.POSITIONS), set(X.POSITIONS) - seen
    assert crafted >= 32 and zeros >= 32
    # the saturating patterns at their four lengths
    sat = {(c.buf, int(c.plen[i])) for c in plan.calls for i in range(c.n) if c.buf.startswith("sat")}
    if layout in ("csr", "seeded"):
        lens = set(plan.calls[0].plen.tolist())
        assert set(X.SAT_LENGTHS) <= lens
    else:
        assert sat == {("sat-" + k, l) for k in X.SAT_PATTERNS for l in X.SAT_LENGTHS}
    if layout == "seeded":
        assert set(X.SEED_STATES[1:]) <= set(plan.calls[2].states.tolist())


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_family_c_differs_outside_the_packets_alone(oracle, layout):
    plan = X.plan(layout, "C", False)
    other = X.alt(plan)
    assert plan.calls[0].n == X.C_PACKETS
    for k, b in plan.bufs.items():
        inside = plan.inside(k)
        assert np.array_equal(b[inside], other.bufs[k][inside])
        assert (b[~inside] ^ other.bufs[k][~inside] == 0xFF).all()
        assert not inside[:X.GUARD].any() and not inside[-X.GUARD:].any()
    assert np.array_equal(X.expect(oracle, plan), X.expect(oracle, other))


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_every_packet_lies_between_the_guards(layout):
    plans = [X.plan(layout, "A", True), X.plan(layout, "A", False), X.plan(layout, "B", False),
             X.plan(layout, "C", False)]
    if layout in ("csr", "seeded", "slotted"):
        plans.append(X.large_plan(layout))
    for p in plans:
        for c in p.calls:
            size = p.bufs[c.buf].size
            assert int(c.start.min()) >= X.GUARD and int((c.start + c.plen).max()) <= size - X.GUARD
            if c.kind == "slotted":                  # the call is handed n whole slots
                assert c.base + c.n * c.stride <= size
            if c.kind in ("csr", "seeded"):
                assert (np.diff(c.offsets) >= 0).all() and c.offsets.size == c.n + 1
                assert c.states is None or c.states.size == c.n


# ---- the expectations discriminate -----------------------------------------------------------------

def _right(pkt, after, start):
    return X.fold(X.word_sum(pkt))


def _mod_fold(pkt, after, start):
    return X.word_sum(pkt) % 0xFFFF                                    # -0 becomes 0


def _tail_low(pkt, after, start):
    if len(pkt) & 1:
        return X.fold(X.word_sum(pkt[:-1]) + int(pkt[-1]))
    return _right(pkt, after, start)


def _one_past(pkt, after, start):
    return X.fold(X.word_sum(np.concatenate([pkt, [after]]).astype(np.uint8)))


def _no_swap(pkt, after, start):
    r = _right(pkt, after, start)
    return (r >> 8 | r << 8) & 0xFFFF if start & 1 else r


def _carry_dropped(pkt, after, start):
    b = np.concatenate([pkt, np.zeros(-len(pkt) % 4, dtype=np.uint8)]).astype(np.uint8)
    s = int(b.view(">u4").sum(dtype=np.uint64)) & 0xFFFFFFFF           # a 32-bit accumulator, no end-around carry
    return X.fold(s)


def _packets(oracle, plan, pick):
    """(packet, the byte behind it, start, length, buffer name, the oracle's inverted sum) of the
    packets `pick` chooses among the unseeded, unfinalised views of the plan's packets."""
    for c in plan.calls:
        b = plan.bufs[c.buf]
        for i in range(c.n):
            s, l = int(c.start[i]), int(c.plen[i])
            if pick(c, i, l):
                yield b[s:s + l], int(b[s + l]), s, l, c.buf, oracle.inverted(b, s, l)


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_wrong_models_disagree_with_the_oracle_in_family_a(oracle, layout):
    """One byte read past the end: at every length of DENSE. The tail byte padded as the low byte
    and an odd start not byte-swapped: somewhere. Each against the oracle's own sum."""
    plan = X.plan(layout, "A", False)
    first = plan.calls[:1] if layout in ("csr", "seeded") else plan.calls
    dense = list(_packets(oracle, X.Plan(plan.bufs, first), lambda c, i, l: l <= 272 and (i < 2 or c.kind != "strided")))
    assert {l for _, _, _, l, _, _ in dense} == set(X.DENSE)
    assert all(_right(p, x, s) == w for p, x, s, l, _, w in dense)       # the local model is the oracle's
    wrong = {l for p, x, s, l, _, w in dense if _one_past(p, x, s) != w}
    assert wrong == set(X.DENSE), sorted(set(X.DENSE) - wrong)
    assert any(_tail_low(p, x, s) != w for p, x, s, l, _, w in dense if l & 1)
    assert any(_no_swap(p, x, s) != w for p, x, s, l, _, w in dense if s & 1)


@pytest.mark.parametrize("layout", X.LAYOUTS)
def test_wrong_models_disagree_with_the_oracle_in_family_b(oracle, layout):
    """The % 0xFFFF fold on the crafted packets; the 32-bit accumulator that drops its carry-out
    on each saturating pattern."""
    plan, marks = X.cached((layout, "B"), lambda: X.plan_b(layout))
    hit = 0
    for k, i, p in marks:
        c = plan.calls[k]
        s, l = int(c.start[i]), int(c.plen[i])
        if p is not None:
            pkt = plan.bufs[c.buf][s:s + l]
            assert _mod_fold(pkt, 0, s) == 0 and oracle.inverted(plan.bufs[c.buf], s, l) == 0xFFFF
            hit += 1
    assert hit
    first = X.Plan(plan.bufs, plan.calls[:1]) if layout in ("csr", "seeded") else plan
    sat = list(_packets(oracle, first, lambda c, i, l: l in X.SAT_LENGTHS and (i < 16 or c.kind != "strided")))
    assert all(_right(p, x, s) == w for p, x, s, l, _, w in sat)
    big = [(p, x, s, w) for p, x, s, l, _, w in sat if l == 65535]
    assert len(big) >= len(X.SAT_PATTERNS)
    for name in X.SAT_PATTERNS:
        ref = X.saturating(name, 65535 + 16)
        mine = [(p, x, s, w) for p, x, s, w in big if np.array_equal(p, ref[s % 16:s % 16 + 65535])]
        assert mine and any(_carry_dropped(p, x, s) != w for p, x, s, w in mine), name
