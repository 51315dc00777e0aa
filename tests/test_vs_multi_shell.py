"""mv.AnalyseN / mv.RecalculateN / mv.DegrainN / mv.CompensateN / mv.MultiField through the VapourSynth filter shell (vsplugin/mvtools_vs.c), which
registers them when the host's environment has MVX_VS_MULTI=1 as the plugin is loaded.

CPU part: the function lists with and without the switch, and the three switches together.  Everything else needs frame 0 of a multi vector clip,
which the test double of the device layer cannot produce, and is a GPU test.

GPU part: whole graphs evaluated through getFrame by one mini-host process per case.  The expected bytes come from the CPU oracle alone
(tests/multi_oracle.py): oracle.Analyse / oracle.Recalculate per field, oracle.Compensate per output, oracle.Degrain up to radius 3 and beyond it the
restatements tests/degrain_n_ref.py / tests/degrain_out16_ref.py fed the oracle's super frames and vectors with thresholds from the formula in Python
(degrain_n_cases.tables) -- never the shell's, the Python package's or the library's.  Comparison is np.array_equal per plane or per blob.
tests/test_vs_multi_cases.py shows on the CPU what the DegrainN and CompensateN cases here rely on."""
import subprocess

import numpy as np
import pytest

import multi_oracle as mu
import pipeline as pl
import test_vs_shim as shim
import vs_multi_cases as vc
from test_vs_shim import HOST, PLUGIN, _read_fmt_frames, _read_frames, _write_clip, host

ANALYSE_TAIL = shim.EXPECTED["Analyse"][len("super:vnode;"):].replace("isb:int:opt;", "").replace("delta:int:opt;", "")
NEW = {
    "AnalyseN": "super:vnode;radius:int;" + ANALYSE_TAIL,
    "RecalculateN": shim.EXPECTED["Recalculate"],
    "DegrainN": "clip:vnode;super:vnode;vectors:vnode;radius:int:opt;thsad:int:opt;thsadc:int:opt;thsad2:int:opt;thsadc2:int:opt;plane:int:opt;limit:int:opt;limitc:int:opt;"
                "thscd1:int:opt;thscd2:int:opt;out16:int:opt;",
    "CompensateN": "clip:vnode;super:vnode;vectors:vnode;tr:int:opt;scbehavior:int:opt;thsad:int:opt;fields:int:opt;time:float:opt;thscd1:int:opt;thscd2:int:opt;tff:int:opt;",
    "MultiField": "vectors:vnode;field:int;",
}
SWITCHES = ("MVX_VS_FLOW", "MVX_VS_DEPAN", "MVX_VS_MULTI")


@pytest.fixture
def multi_on(monkeypatch):
    monkeypatch.setenv("MVX_VS_MULTI", "1")  # (proc_env() copies os.environ)


def _listed():
    out = host("list").splitlines()
    assert out[0] == "id=com.nodame.mvtools ns=mv"
    return dict(line.split(" ", 1) for line in out[1:])


# ---------------------------------------------------------------------------------------------------- CPU

def test_the_argument_strings_are_the_single_filters_without_isb_and_delta():
    assert "isb" not in NEW["AnalyseN"] and "delta" not in NEW["AnalyseN"]
    assert NEW["AnalyseN"].count(";") == shim.EXPECTED["Analyse"].count(";") - 2 + 1
    assert NEW["RecalculateN"].startswith("super:vnode;vectors:vnode;thsad:int:opt;")


def test_switch_registers_exactly_the_five_filters(monkeypatch, multi_on):
    for s in SWITCHES[:2]:
        monkeypatch.delenv(s, raising=False)
    assert _listed() == dict(shim.EXPECTED, **NEW)


def test_without_the_switch_the_interface_is_unchanged(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    assert _listed() == shim.EXPECTED
    monkeypatch.setenv("MVX_VS_MULTI", "0")
    assert _listed() == shim.EXPECTED


@pytest.mark.parametrize("on", [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)], ids=lambda on: "flow%d-depan%d-multi%d" % on)
def test_the_three_switches_are_independent(monkeypatch, on):
    import test_vs_depan_shell as depan
    import test_vs_flow_shell as flow
    for s, v in zip(SWITCHES, on):
        monkeypatch.setenv(s, str(v))
    want = dict(shim.EXPECTED)
    for new, v in zip((flow.NEW, depan.NEW, NEW), on):
        if v:
            want.update(new)
    got = _listed()
    assert got == want
    assert any(k.startswith("Depan") for k in got) == bool(on[1])   # in particular: MVX_VS_MULTI=1 alone registers no Depan function


# ---------------------------------------------------------------------------------------------------- GPU: graphs against the oracle

gpu = pytest.mark.gpu


class Graph:
    """an oracle-side multi clip (tests/multi_oracle.py) on disk, and mini-host runs over it"""

    def __init__(self, m, tmp_path):
        self.m, self.dir = m, tmp_path
        self.src = tmp_path / "in.raw"
        _write_clip(self.src, m.frames)

    def cli(self, margs=None, rargs=None, fargs=None, *extra):
        m = self.m
        out = ["s.%s=%s" % kv for kv in m.skw.items()] + ["m.radius=%d" % m.radius] + ["m.%s=%s" % kv for kv in dict(m.akw, **(margs or {})).items()]
        out += ["r.%s=%s" % kv for kv in (rargs or {}).items()] + ["f.%s=%s" % kv for kv in (fargs or {}).items()]
        if m.fmt != "420":
            out.append("x.format=" + m.fmt)
        return out + list(extra)

    def run(self, pipeline, *cli, name="out.raw", env=None, check=True):
        """one mini-host process; returns (CompletedProcess, path of the result file)"""
        m = self.m
        path = self.dir / name
        cmd = [HOST, PLUGIN] + [str(a) for a in ("run", pipeline, self.src, m.w, m.h, m.bits, m.n, path)] + list(cli)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=shim.proc_env(**(env or {})))
        if check:
            assert r.returncode == 0 and "DONE" in r.stdout, r.stdout + r.stderr
        return r, path

    def read(self, path, n, bits=None):
        m = self.m
        bits = m.bits if bits is None else bits
        return _read_frames(path, m.w, m.h, bits, n) if m.fmt == "420" else _read_fmt_frames(path, m.w, m.h, bits, n, m.fmt)


def _same(got, want, what):
    assert len(got) == len(want), what
    for n, (g, w) in enumerate(zip(got, want)):
        if w is None:
            continue
        assert len(g) == len(w), (what, n)
        for p in range(len(w)):
            assert g[p].shape == w[p].shape and g[p].dtype == w[p].dtype, (what, n, p, g[p].shape, w[p].shape)
            assert np.array_equal(g[p], w[p]), "%s frame %d plane %d: %s" % (what, n, p, pl.first_diff(g[p], w[p]))


def _fields_equal(got, ads, blobs, what):
    for n, row in enumerate(got):
        for r, (ad, blob) in enumerate(row):
            assert ad == bytes(ads[r]), "%s frame %d field %d: analysis data" % (what, n, r)
            assert np.array_equal(blob, blobs[n][r]), "%s frame %d field %d: %s" % (what, n, r, pl.first_diff(blob, blobs[n][r]))


# ---- AnalyseN and MultiField

@gpu
@pytest.mark.parametrize("case", vc.ANALYSE_CASES, ids=vc.analyse_id)
def test_multianalyse_fields_are_oracle_analyse(multi_on, oracle, tmp_path, case):
    m = vc.analyse_multi(case)
    g = Graph(m, tmp_path)
    r, path = g.run("multianalyse", *g.cli())
    stride = (m.blobs[0][0].size + 255) // 256 * 256
    assert r.stdout.splitlines()[0] == "multi radius=%d stride=%d" % (m.radius, stride)
    _fields_equal(mu.fields_of_dump(open(path, "rb").read(), m.n, 2 * m.radius), m.ads, m.blobs, "multianalyse")
    assert m.blobs[0][0].size < stride
    # the whole property: the fields at their strides, every pad byte 0
    _, path = g.run("multianalyse", *g.cli(None, None, None, "x.dump=prop"), name="prop.raw")
    prop = np.fromfile(path, dtype=np.uint8).reshape(m.n, 2 * m.radius, stride)
    for n in range(m.n):
        for f in range(2 * m.radius):
            size = m.blobs[n][f].size
            assert np.array_equal(prop[n, f, :size], m.blobs[n][f]) and not prop[n, f, size:].any(), (n, f)
    valid = sum(int(m.blobs[n][f][4:8].view(np.int32)[0]) for n in range(m.n) for f in range(2 * m.radius))
    assert valid == m.n * 2 * m.radius - m.radius * (m.radius + 1)  # (both clip ends are in the run)


@gpu
@pytest.mark.parametrize("case,field", vc.FIELD_CASES, ids=lambda v: vc.analyse_id(v) if isinstance(v, tuple) else "field%d" % v)
def test_multifield_is_an_ordinary_vector_clip_of_that_field(multi_on, oracle, tmp_path, case, field):
    m = vc.analyse_multi(case)
    g = Graph(m, tmp_path)
    _, path = g.run("multifield", *g.cli(None, None, dict(field=field)))
    got = mu.fields_of_dump(open(path, "rb").read(), m.n, 1)
    _fields_equal(got, [m.ads[field]], [[m.blobs[n][field]] for n in range(m.n)], "multifield")


# ---- RecalculateN

@gpu
@pytest.mark.parametrize("case", vc.RECALC_CASES, ids=mu.recalc_id)
def test_multirecalculate_fields_are_oracle_recalculate(multi_on, oracle, tmp_path, case):
    m = mu.recalc_multi(case)
    rkw = mu.recalc_kwargs(case)
    ads, blobs = m.recalc(**rkw)
    g = Graph(m, tmp_path)
    r, path = g.run("multirecalculate", *g.cli(None, rkw))
    stride = (blobs[0][0].size + 255) // 256 * 256
    assert r.stdout.splitlines()[0] == "multi radius=%d stride=%d" % (m.radius, stride)
    _fields_equal(mu.fields_of_dump(open(path, "rb").read(), m.n, 2 * m.radius), ads, blobs, "multirecalculate")
    _, path = g.run("multirecalculate", *g.cli(None, rkw, None, "x.dump=prop"), name="prop.raw")
    prop = np.fromfile(path, dtype=np.uint8).reshape(m.n, 2 * m.radius, stride)
    size = blobs[0][0].size
    assert size < stride and not prop[:, :, size:].any()


# ---- DegrainN

@gpu
@pytest.mark.parametrize("case", vc.DEGRAIN_CASES, ids=vc.degrain_id)
def test_multidegrain_frames(multi_on, oracle, tmp_path, case):
    m = vc.degrain_multi(case)
    fargs, rkw = case[8], case[9]
    g = Graph(m, tmp_path)
    want = vc.degrain_expected(oracle, case)
    _, path = g.run("multidegrain", *g.cli(None, rkw, fargs))
    got = g.read(path, m.n, bits=16 if fargs.get("out16") else None)
    _same(got, want, "DegrainN")
    checked = [n for n, w in enumerate(want) if w is not None]
    assert m.n // 2 in checked and 0 in checked and m.n - 1 in checked
    src = m.frames[m.n // 2][0]
    src = src.astype(np.uint16) << 8 if fargs.get("out16") else src
    assert not np.array_equal(got[m.n // 2][0], src)


# ---- CompensateN

@gpu
@pytest.mark.parametrize("case", vc.COMPENSATE_CASES, ids=vc.compensate_id)
def test_multicompensate_frames(multi_on, oracle, tmp_path, case):
    m = vc.compensate_multi(case)
    tr, fargs, extra, env = vc.compensate_tr(case), case[5], case[6], case[7]
    g = Graph(m, tmp_path)
    want = vc.compensate_expected(oracle, case)
    no = 2 * tr + 1
    r, path = g.run("multicompensate", *g.cli(None, None, fargs, *extra), env=env)
    lines = r.stdout.splitlines()
    assert lines[0] == "multicompensate frames=%d fps=%d/1" % (m.n * no, 24 * no)
    assert "frame1 _DurationNum=1 _DurationDen=%d" % (24 * no) in lines   # std.AssumeFPS ran
    assert "permits out" not in r.stderr, r.stderr
    got = g.read(path, m.n * no)
    _same(got, want, "CompensateN")
    for n in range(m.n):
        for p in range(len(m.frames[n])):
            assert np.array_equal(got[n * no + tr][p], m.frames[n][p]), "the centre of frame %d" % n
    moved = sum(not np.array_equal(got[n * no + k][0], m.frames[n][0]) for n in range(m.n) for k in range(no))
    assert moved >= tr or "thscd1" in fargs


# ---- creation

MF = "Property 'MVTools_MVAnalysisData' not found in first frame of "
ERRORS = [
    (("AnalyseN", "f.radius=0"), "AnalyseN: radius must be between 1 and 24."),
    (("AnalyseN", "f.radius=25"), "AnalyseN: radius must be between 1 and 24."),
    (("AnalyseN", "f.radius=2", "f.blksize=7"), None),
    (("AnalyseN", "f.radius=2", "f.isb=1"), "AnalyseN: Function does not take argument(s) named isb"),
    (("RecalculateN", "m.radius=2", "f.search=9"), "RecalculateN: search must be between 0 and 7 (inclusive)."),
    (("DegrainN", "m.radius=2", "f.radius=3"), "DegrainN: radius is greater than the radius of the vector clip."),
    (("DegrainN", "m.radius=2", "f.radius=0"), "DegrainN: radius must be between 1 and 24."),
    (("DegrainN", "m.radius=2", "f.plane=5"), "DegrainN: plane must be between 0 and 4 (inclusive)."),
    (("CompensateN", "m.radius=2", "f.tr=3"), "CompensateN: tr is greater than the radius of the vector clip."),
    (("CompensateN", "m.radius=2", "f.tr=0"), "CompensateN: tr must be between 1 and 24."),
    (("CompensateN", "m.radius=2", "f.fields=1"), "CompensateN: fields is not supported."),
    (("CompensateN", "m.radius=2", "f.time=101.0"), "CompensateN: time must be between 0.0 and 100.0 (inclusive)."),
    (("MultiField", "m.radius=2", "f.field=4"), "MultiField: field must be between 0 and 3."),
    (("MultiField", "m.radius=2", "f.field=-1"), "MultiField: field must be between 0 and 3."),
    # a multi vector clip where a single-field one belongs, in that filter's own words
    (("Degrain1", "m.radius=2", "x.vectors=multi"), "Degrain1: " + MF + "mvbw."),
    (("Compensate", "m.radius=2", "x.vectors=multi"), "Compensate: " + MF + "vectors."),
    # ... and an ordinary vector clip where a multi one belongs
    (("DegrainN", "x.vectors=single"), "DegrainN: Property 'MVTools_multi_MVAnalysisData' not found in first frame of vectors."),
    (("CompensateN", "x.vectors=single"), "CompensateN: Property 'MVTools_multi_MVAnalysisData' not found in first frame of vectors."),
    (("MultiField", "x.vectors=single", "f.field=0"), "MultiField: Property 'MVTools_multi_MVAnalysisData' not found in first frame of vectors."),
    # a clip that is not the one the super clip was made from
    (("DegrainN", "m.radius=2", "x.clip=144x96x8"), "DegrainN: wrong source or super clip frame size."),
    (("DegrainN", "m.radius=2", "x.clip=128x96x16"), "DegrainN: wrong source or super clip frame size."),
    (("CompensateN", "m.radius=2", "x.clip=144x96x8"), "CompensateN: wrong source or super clip frame size."),
]


@gpu
@pytest.mark.parametrize("args,msg", ERRORS, ids=lambda v: "-".join(v) if isinstance(v, tuple) else None)
def test_creation_errors(multi_on, args, msg):
    out = host("error", args[0], 128, 96, 8, *args[1:]).strip()
    if msg is None:
        assert out.startswith("ERROR AnalyseN: the block size must be")
    else:
        assert out == "ERROR " + msg


@gpu
def test_out16_needs_an_8_bit_clip(multi_on):
    assert host("error", "DegrainN", 128, 96, 16, "m.radius=2", "f.out16=1").strip() == "ERROR DegrainN: out16 needs an 8 bit clip."
    assert host("error", "DegrainN", 128, 96, 8, "m.radius=2", "f.out16=1").strip() == "OK 128x96 frames=4"


@gpu
def test_output_clip_info(multi_on):
    assert host("error", "AnalyseN", 128, 96, 8, "f.radius=3").strip().endswith("frames=4")
    assert host("error", "RecalculateN", 128, 96, 8, "m.radius=3", "f.blksize=4").strip().endswith("frames=4")
    assert host("error", "MultiField", 128, 96, 8, "m.radius=3", "f.field=5").strip().endswith("frames=4")
    assert host("error", "DegrainN", 128, 96, 8, "m.radius=3", "f.radius=2").strip() == "OK 128x96 frames=4"
    assert host("error", "CompensateN", 128, 96, 8, "m.radius=3").strip() == "OK 128x96 frames=28"
    assert host("error", "CompensateN", 128, 96, 8, "m.radius=3", "f.tr=1").strip() == "OK 128x96 frames=12"
    # every existing filter takes a field through mv.MultiField: the CompensateN pipeline's `vectors` is again a multi clip for DegrainN
    assert host("error", "DegrainN", 128, 96, 16, "m.radius=1", "x.format=444").strip() == "OK 128x96 frames=4"


def test_without_the_switch_the_filters_do_not_exist(monkeypatch):
    monkeypatch.delenv("MVX_VS_MULTI", raising=False)
    assert host("error", "AnalyseN", 128, 96, 8, "f.radius=2").strip() == "ERROR no function AnalyseN"
    assert host("error", "DegrainN", 128, 96, 8, "m.radius=2", check=False).strip() == "ERROR AnalyseN: no function AnalyseN"   # (the mini host builds the vector clip first)
