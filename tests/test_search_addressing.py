"""CPU audit of the search kernels' reference addressing (no GPU): csrc/mvx_analyse_addr.h -- the one text the lean kernel, the speculative
kernel and the specialised general kernels take their unsigned 32-bit offsets from -- walked on the host by
tests/search_addressing_host_main.cpp (its own main, AddressSanitizer + UBSan) over the level tables the library itself makes
(mvx_analyse_debug_level), for every level, block and loadable vector of a grid of geometries: base + (u32 offset) must equal the signed
64-bit truth and stay inside the plane's promised bytes.

The grid holds the search that faulted on a GPU (8-bit 36x36 Gray, no padding) and its relatives with an EMPTY legal rectangle on the
coarsest level, where the clipped predictors lie left of and above the level's first sample.  Built with the bias switched off
(-DMVX_REF_BIAS_ROWS=0 -DMVX_REF_BIAS_COLS=0: the arithmetic before the bias) the program must report that case as a wrap of 2^32 on row 0;
profiles/small_geometry_addressing.txt keeps both outputs."""
import os
import re
import subprocess

import pytest

import small_geometry_cases as sg

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vapoursynth-mvtools_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def describe(mv, g):
    """the program's input for one geometry, or None when the library refuses it (with the message)"""
    try:
        sup, an = sg.make(mv, g)
    except mv.MvtoolsError as e:
        return None, str(e)
    lv = an.levels()
    rng = [sup.shadow_stride[p] * sup.slots[p] if sup.shadow else sup.info.plane_height[p] * sup.pitch[p] for p in range(sup.nplanes)]
    chroma = 0 if g["fmt"] == "gray" else int(g["akw"].get("chroma", 1))
    head = "G %s %d %d %d %d %d %d %d %d" % (g["name"], sup.bps, chroma, g["akw"]["blksize"], g["akw"]["overlap"], lv[0][23], rng[0], rng[1] if len(rng) > 1 else 0, len(lv))
    return "\n".join([head] + ["L " + " ".join(str(v) for v in row) for row in lv]) + "\n", None


@pytest.fixture(scope="module")
def audit(tmp_path_factory):
    """the two builds of the program: the header as the kernels compile it, and with the bias off"""
    tmp = tmp_path_factory.mktemp("search_addressing")
    exes = {}
    for tag, defs in (("biased", []), ("unbiased", ["-DMVX_REF_BIAS_ROWS=0", "-DMVX_REF_BIAS_COLS=0"])):
        exes[tag] = str(tmp / ("search_addressing_" + tag))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I" + CSRC, os.path.join(HERE, "search_addressing_host_main.cpp"), "-o", exes[tag]] + SAN + defs)

    def run(tag, text):
        r = subprocess.run([exes[tag]], input=text, capture_output=True, text=True)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-4000:]
        return r.returncode, r.stdout
    return run


@pytest.fixture(scope="module")
def grid(mv):
    texts, refused = {}, {}
    for g in sg.audit_grid():
        t, why = describe(mv, g)
        if t is None:
            refused[g["name"]] = why
        else:
            texts[g["name"]] = t
    return texts, refused


@pytest.fixture(scope="module")
def biased_run(audit, grid):
    return audit("biased", "".join(grid[0].values()))


def test_the_kernels_take_their_offsets_from_the_audited_header():
    """one text: no kernel header forms a sub-pel plane offset of its own any more"""
    own = re.compile(r"\(unsigned\)\(a[xy] >> logPel\)")
    for name in ("mvx_analyse_fast.h", "mvx_analyse_spec.h", "mvx_analyse_kernel.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert not own.search(text), name
        assert "mvx_luma_off32<BPS>" in text and "mvx_chroma_off32<BPS>" in text and "mvx_ref_bias_bytes" in text, name
        assert "mvx_piece_off32(" in text and "mvx_rows_step32(" in text, name
    assert len(own.findall(open(os.path.join(CSRC, "mvx_analyse_addr.h")).read())) == 2


def test_grid_holds_what_it_must(mv, oracle, grid):
    texts, refused = grid
    assert len(texts) > 500
    for g in sg.EMPTY + sg.ORDINARY:
        assert g["name"] in texts, (g["name"], refused.get(g["name"]))
    route = {n: int(t.split()[6]) for n, t in texts.items()}
    assert all(route[g["name"]] == 2 for g in sg.EMPTY)                     # the lean / speculative kernels run them
    assert all(route[g["name"]] >= 1 for g in sg.ORDINARY)                  # (pel 4 searched at pelsearch 4: the specialised general kernels only)
    assert route["35x30-444-8bit-pel2-pad0.0-blk8.4"] == 0                  # 4:4:4: the generic kernel, 64-bit addresses
    names = " ".join(texts)
    for part in ("pad1.1", "pad2.0", "pel1", "pel2", "pel4", "blk8.4", "blk8.0", "blk16.8", "blk16.0", "16bit-pel2-pad0.0-blk32.16", "noshadow", "-gray-", "-420-"):
        assert part in names, part
    # what is refused is refused by the oracle too
    for g in sg.audit_grid():
        if g["name"] in refused:
            with pytest.raises(oracle.OracleError):
                sg.make(oracle, g)


def test_audit_is_clean_over_the_grid(biased_run):
    rc, out = biased_run
    assert rc == 0 and "VIOLATION" not in out, [l for l in out.splitlines() if l.startswith("VIOLATION")][:5]
    assert out.splitlines()[-1].startswith("search_addressing_host_main: 0 of ")


def test_grid_really_contains_empty_rectangles(biased_run):
    """nDxMax <= nDxMin and nDyMax <= nDyMin on some level of every case listed as empty -- else the audit would prove nothing about them"""
    _, out = biased_run
    empty = {}
    for line in out.splitlines():
        m = re.match(r"level (\S+) (\d+) emptyx=(\d+) emptyy=(\d+)", line)
        if m:
            e = empty.setdefault(m.group(1), [0, 0])
            e[0] += int(m.group(3)); e[1] += int(m.group(4))
    for g in sg.EMPTY:
        assert empty[g["name"]][0] > 0 and empty[g["name"]][1] > 0, (g["name"], empty[g["name"]])
    for g in sg.ORDINARY + sg.FULL_PAD0:
        assert empty[g["name"]] == [0, 0], g["name"]
    assert sum(1 for e in empty.values() if e[0] and e[1]) >= 90  # (the 36x36 geometries of the grid: 8 / 16 bits, Gray / 4:2:0, pel, padding, blocks)


def test_the_arithmetic_before_the_bias_wraps_on_the_search_that_faulted(audit, grid):
    """the cause of the GPU fault, found without a GPU: row 0 of the clipped predictor (-1, -1) of the coarsest level's one block"""
    texts, _ = grid
    rc, out = audit("unbiased", texts[sg.FAULTING["name"]])
    lines = [l for l in out.splitlines() if l.startswith("VIOLATION")]
    assert rc == 1 and len(lines) == 1, out
    f = dict(kv.split("=", 1) for kv in lines[0].split()[1:])
    assert f["level"] == "2" and f["block"] == "(0,0)" and f["vector"] == "(-1,-1)" and f["row"] == "0" and f["plane"] == "0" and int(f["diff"]) == 1 << 32, lines[0]
    # ... and every case with an empty rectangle has it; the ordinary padded geometries never did
    for g in sg.EMPTY:
        rc, out = audit("unbiased", texts[g["name"]])
        assert rc == 1 and "diff=4294967296" in out, g["name"]
    rc, out = audit("unbiased", "".join(texts[g["name"]] for g in sg.ORDINARY))
    assert rc == 0 and "VIOLATION" not in out, out[-2000:]


def test_single_block_clip_is_refused_by_library_and_oracle_alike(mv, oracle, grid):
    """16x16, one 16x16 block, pel 1, no padding, one level: a block as large as the padded frame has an empty legal rectangle on the FINEST level, and
    the clipped predictor (-1, -1) would be read one row and one sample in front of the caller's plane itself.  Both refuse it, in the same words; one
    sample of padding, or one more sample of frame, makes it a clip like any other -- and the audit takes those."""
    texts, refused = grid
    words = "Analyse: the padded frame must be larger than a block (no vector is legal otherwise)."
    assert refused[sg.SINGLE_BLOCK["name"]] == words
    with pytest.raises(oracle.OracleError, match="the padded frame must be larger than a block"):
        sg.make(oracle, sg.SINGLE_BLOCK)
    for g in sg.NEARLY_SINGLE:
        assert g["name"] in texts, refused.get(g["name"])
        sg.make(oracle, g)


def test_restated_row_pass_starts_are_the_kernels_text():
    """the host program restates where a lane of a row pass starts (the header holds the offsets, not these): the expressions must stand in
    mvx_analyse_spec.h word for word, so that neither side drifts"""
    norm = lambda t: re.sub(r"\s+", " ", t.replace("std::min", "min"))
    kernel = norm(open(os.path.join(CSRC, "mvx_analyse_spec.h")).read())
    host = norm(open(os.path.join(HERE, "search_addressing_host_main.cpp")).read())
    for both in ("const int qe = min(qS, (nd - 1) >> 2), d0 = min(4 * qe, nd - 4);",
                 "xl + 16 > pw ? 2 : 0", "xc + 16 > pw ? 2 : 0",
                 "xc = 2 * ((((bx0 >> 1) << logPel) + ((vx + (vx < 0 ? 1 : 0)) >> 1)) >> logPel)",
                 "xl = ((bx0 << logPel) + vx) >> logPel"):
        assert both in kernel, both
        assert both.replace("bx0", "x0").replace("vx", "v.first") in host or both in host, both
    # the kernel's forms with its own names, and the host's with the same constants spelled out (TC = blocks' column step, HC = 1, LV = the window's blocks)
    assert "const int pe = min(p, TC * (LV - 1) + 2 * HC - 1) * COLB;" in kernel and "const int pe = min(p, tc * (Lw - 1) + 1) * colb;" in host
    assert "const int nd = ds2 ? 2 * L : L + 1;" in kernel and "const int nd = side ? 2 * Lw : Lw + 1;" in host
    assert "(a window has at least four dwords: groups of one or two blocks go one block at a time)" in kernel
