"""CPU: the scripts of tests/test_gpu_handle_sequences.py test what they claim.  From the oracle alone, for every adapter: the jobs of a script
have pairwise different outputs on every plane the handle writes (a handle that answered a call with another job's records could not pass), S
is unusable in every vector field, S2 in exactly one (or, where a job's fields belong together, it is a second unusable job), U and V are
usable and compensate most of their blocks, the mask modes of BlockFPS really change U's output, and the calls have the sizes that make a
handle free, regrow and reuse its scratch.  These are conditions that the clip's seed and cut were chosen to meet, not measurements."""
import numpy as np
import pytest

import handle_sequences as hs
import multi_cases as mc

LETTERS = ("U", "V", "S", "E", "S2")
ADAPTERS = pytest.mark.parametrize("adapter", hs.ADAPTERS, ids=lambda a: a.name)


@ADAPTERS
def test_the_jobs_of_a_script_have_pairwise_different_outputs(adapter):
    letters = [l for l in adapter.jobs]
    want = {l: adapter.expect(l) for l in letters}
    planes = adapter.writes_planes if adapter.writes_planes is not None else range(len(want["U"]))
    for i, a in enumerate(letters):
        for b in letters[i + 1:]:
            if a in adapter.alike and b in adapter.alike:
                continue
            for p in planes:
                if want[a][p].shape != want[b][p].shape:  # (a single blob and a multi blob)
                    continue
                assert not np.array_equal(want[a][p], want[b][p]), "jobs %s and %s give the same output %d" % (a, b, p)


@pytest.mark.parametrize("adapter", [a for a in hs.ADAPTERS if a.vectors], ids=lambda a: a.name)
def test_usable_and_unusable_jobs_are_what_their_names_say(adapter):
    w, ad = adapter.world, adapter.field_ad()
    th = {k: v for k, v in adapter.kw.items() if k in ("thscd1", "thscd2")}

    def usable(letter):
        return [present and w.usable(blob, ad, **th) for blob, present in adapter.fields(letter)]

    assert len(adapter.fields("U")) == adapter.nfields
    assert not any(usable("S"))
    if adapter.partial:  # the launch of five mixes at least three counts of usable references; U and V have three or more
        counts = {l: sum(usable(l)) for l in hs.CALL3}
        assert len(set(counts.values())) >= 3, counts
        assert min(counts["U"], counts["V"]) >= 3, counts
        assert counts["S2"] >= 1 and any(present and not u for (_, present), u in zip(adapter.fields("S2"), usable("S2")))
        first = {l: w.below_thsad(adapter.fields(l)[0][0], adapter.thsad, ad) for l in ("U", "V")}
        assert min(first.values()) >= mc.USED, first
        return
    assert all(usable("U")) and all(usable("V"))
    assert all(present for _, present in adapter.fields("S")) and all(present for _, present in adapter.fields("S2")), "S and S2 are scene changes, not clip ends"
    assert not all(present for _, present in adapter.fields("E") + adapter.extra_fields("E"))
    if adapter.s2_one_direction:
        assert sorted(usable("S2")) == [False, True]
        if isinstance(adapter, hs.DegrainAdapter):
            assert sum(usable("E")) == 1, "the clip end leaves one usable reference"
    else:
        assert not any(usable("S2"))
    if adapter.cut == "partial":  # the usable flag decides: without it the matching blocks of S and S2 would be used
        for letter in ("S", "S2"):
            shares = [w.below_thsad(blob, adapter.thsad, ad) for (blob, _), u in zip(adapter.fields(letter), usable(letter)) if not u]
            assert shares and min(shares) >= hs.MATCHING, "%s: only %.3f of an unusable field's blocks are below thsad" % (letter, min(shares))
    if adapter.thsad is not None:
        for letter in ("U", "V"):
            shares = [w.below_thsad(blob, adapter.thsad, ad) for blob, _ in adapter.fields(letter)]
            assert min(shares) >= mc.USED, "%s compensates only %.3f of its blocks" % (letter, min(shares))
            if adapter.thsad < 400:  # the handle whose thsad is there to make blocks fall back
                assert max(shares) <= 1 - mc.UNUSED, "%s falls back on only %.3f of its blocks" % (letter, 1 - max(shares))


@pytest.mark.parametrize("adapter", [a for a in hs.ADAPTERS if isinstance(a, hs.BlockFPSAdapter) and a.kw.get("mode", 0) >= 3], ids=lambda a: a.name)
def test_blockfps_masks_change_the_usable_jobs(adapter):
    """the occlusion masks (modes 3 and above; dSmall in mvx_blockfps_frames) are not all zero on U and V: without them the output is mode 0's
    (a mode whose masks were empty could not tell a stale mask from a fresh one)"""
    plain = hs.BlockFPSAdapter("plain", adapter.shape, adapter.fmt, mode=0)
    for letter in ("U", "V"):
        assert hs.differing(adapter.expect(letter), plain.expect(letter)), letter
    kw = dict(adapter.kw, ml=adapter.kw["ml"] * 4)
    other = hs.BlockFPSAdapter("other-ml", adapter.shape, adapter.fmt, **kw)
    assert hs.differing(adapter.expect("U"), other.expect("U")), "ml does not matter: the masks are saturated or empty"


@pytest.mark.parametrize("adapter", [a for a in hs.ADAPTERS if isinstance(a, hs.MaskAdapter)], ids=lambda a: a.name)
def test_the_masks_of_the_usable_jobs_are_not_empty(adapter):
    """a stale mask could not be told from a fresh one if U's were flat; an unusable frame's planes hold the fill value, which no plane of U does"""
    kind = adapter.kw["kind"]
    planes = [0] if kind <= 2 else [1, 2] if kind <= 4 else [1, 2]  # kinds 0-2 write the mask to the luma (and its copy to the chroma), 3-5 the vector components to the chroma
    for letter in ("U", "V"):
        for p in planes:
            assert len(np.unique(adapter.expect(letter)[p])) >= 8, (letter, p)
    fill = adapter.expect("S")[1]
    assert len(np.unique(fill)) == 1 and np.array_equal(fill, adapter.expect("S2")[1])


@ADAPTERS
def test_the_calls_free_regrow_and_reuse_the_scratch(adapter):
    script = adapter.script()
    n = [len(letters) for letters, _ in script]
    assert script[:9] == hs.STANDARD
    assert n[0] == 1 and n[1] == 0 and n[2] > 2 * n[0], "call 3 must outgrow the headroom of call 1 (twice its jobs)"
    assert n[3] < n[2] and n[4] <= n[2] and n[5] == 1
    assert script[4][0] == tuple(reversed([l for l in script[2][0] if l in script[4][0]])), "call 5 holds jobs of call 3 in the other order"
    assert script[5] == script[0]
    assert [s for _, s in script[6:9]] == [1, 2, 1] and [l for l, _ in script[6:9]] == [l for l, _ in script[2:5]]
    for letters, _ in script:
        assert all(l in adapter.jobs for l in letters)
    assert script[-len(hs.SWAP):] == hs.SWAP and hs.SWAP[0][0] == tuple(reversed(hs.SWAP[1][0])) and len(hs.SWAP[0][0]) <= n[2]
    if isinstance(adapter, hs.BlockFPSAdapter):  # time256 0, 128 and 256 in one launch, beside an unusable job
        times = [[adapter._ob().map(adapter.jobs[l])[2] for l in letters] for letters, _ in script]
        assert any({0, 128, 256} <= set(t) and "S" in letters for t, (letters, _) in zip(times, script))
        last = adapter.world.floats()[0] if isinstance(adapter, hs.BlockFPSFloatAdapter) else adapter.world.frames
        assert not hs.differing(adapter.expect("T256"), last[3]) and not hs.differing(adapter.expect("T0"), last[6])
    if isinstance(adapter, hs.FlowAdapter) and adapter.fps:  # a copy job and several times in one launch, beside an unusable job
        times = [[adapter._ref().map(adapter.jobs[l])[2] for l in letters] for letters, _ in script]
        assert any(0 in t and len(set(t)) >= 3 and "S" in letters for t, (letters, _) in zip(times, script))
        assert len(set(times[2])) >= 3


@pytest.mark.parametrize("adapter", [a for a in hs.ADAPTERS if isinstance(a, hs.FlowAdapter)], ids=lambda a: a.name)
def test_the_flow_jobs_take_the_formulas_and_fallbacks_they_are_there_for(adapter):
    """U and V take their handle's interpolation formula with non-empty occlusion masks (another ml gives another picture), S and S2 the
    fallback; with both pairs of vectors in use (FlowInter, FlowFPS mask 2) E lacks the extra pair and takes the other formula"""
    kinds = {l: adapter.kind(l).replace("128", "") for l in adapter.jobs}
    fallback = "blend" if adapter.kw.get("blend", 1) else "left"
    both = not adapter.fps or adapter.kw.get("mask") == 2
    main = "extra" if both else "regular" if adapter.kw.get("mask") == 1 else "simple"
    assert kinds["U"] == kinds["V"] == main and kinds["S"] == kinds["S2"] == fallback, kinds
    if adapter.fps:
        assert kinds["T0"] == "copy" and kinds["E"] == ("simple" if both else main), kinds
    else:
        assert kinds["E"] == fallback, kinds
    other = hs.FlowAdapter("other-ml", adapter.shape, adapter.fmt, **dict(adapter.kw, ml=adapter.kw.get("ml", 100.0) / 3))
    for l in ("U", "V"):
        assert hs.differing(adapter.expect(l), other.expect(l)), "%s: ml does not matter, the occlusion masks are empty" % l


@pytest.mark.parametrize("adapter", [a for a in hs.ADAPTERS if type(a) is hs.AnalyseAdapter], ids=lambda a: a.name)
def test_the_analyse_script_comes_round_to_every_job_table_with_other_counts(adapter):
    """a call without jobs returns before it takes a table (mvx_analyse_frames), so the tables go round over the calls that have jobs"""
    counts = [len(letters) for letters, _ in adapter.script() if letters]
    assert len(counts) > 2 * hs.KSLOTS
    for slot in range(hs.KSLOTS):
        seq = counts[slot::hs.KSLOTS]
        assert len(seq) >= 3
        grown = any(b > 2 * max(seq[:i + 1]) for i, b in enumerate(seq[1:]))
        fewer = any(b < max(seq[:i + 1]) for i, b in enumerate(seq[1:]))
        assert grown or fewer, (slot, seq)
        assert seq[0] == seq[1], "the table is first reused as it was left"
    slots = [counts[s::hs.KSLOTS] for s in range(hs.KSLOTS)]
    assert sum(any(b > 2 * max(seq[:i + 1]) for i, b in enumerate(seq[1:])) for seq in slots) >= 2
    assert sum(any(b < max(seq[:i + 1]) for i, b in enumerate(seq[1:])) for seq in slots) >= 2
