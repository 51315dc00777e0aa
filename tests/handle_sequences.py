"""What the handle-sequence tests share (test infrastructure): one driver that runs a SCRIPT -- a list of calls of unlike jobs, some on
other streams -- on ONE handle of a filter, and one adapter per handle type.

Every *_frames entry point works on device scratch that its handle owns and keeps between calls (job tables, usable flags, plans, masks);
it is never cleared, and it grows with headroom.  The contract is "each kernel writes what the next one reads, for this call's jobs only".
A kernel that read a record, a flag or a mask byte of a job that this call did not write would go unnoticed by tests that make a fresh handle
for every call: there the bytes are zero, or equal to what the call would have written.  The scripts here follow a usable job with an
unusable one in the same slot, grow a handle's buffers past their headroom and shrink the call again, and swap jobs between slots; with
mvx_debug_option("scratch_poison", byte) every fresh allocation holds that byte instead of zeros.

The clip: 10 frames of pipeline.moving_clip, frame 5 replaced by uniform noise (the planted scene change; cut="partial": only its upper
five eighths, for the Degrain handles that must tell an unusable reference from one whose blocks all weigh nothing).  Jobs are named by letter:
    U   every reference usable                V   the same on other frames
    S   every vector field unusable (across the cut)
    E   a reference outside the clip (null pointers, the invalid blob)
    S2  unusable in one direction only (filters with one vector field per job, or whose two fields belong to one pair of frames: a second
        unusable job on other frames)
The expected output of a job comes from the CPU oracle, once per adapter and job; inputs of the handle under test (super frames, vectors) are
the oracle's, so a script isolates its handle."""
import ctypes as C
import functools

import numpy as np

import pipeline as pl
import vector_fields

NFRAMES, CUT = 10, 5
KSLOTS = 4  # mvx_analyse::kSlots (csrc/mvx_analyse.hip): the rotating job tables of one Analyse handle

SHAPES = {
    "8bit-blk8-ov4": (128, 96, 8, dict(blksize=8, overlap=4)),
    "16bit-blk16-ov8": (192, 112, 16, dict(blksize=16, overlap=8)),
    "8bit-blk8-ov0": (206, 118, 8, dict(blksize=8, overlap=0)),   # the side-by-side cell kernel; 6 columns and 6 rows that no block covers
}
FORMATS = {"420": {}, "444": dict(subsampling=(0, 0)), "gray": dict(gray=True)}

# (jobs by letter, stream): stream 0 is the caller's current stream and is waited for after the call; 1 and 2 are two other streams, whose
# calls follow each other without any host synchronisation (CallGuard's stream wait is all that orders them on the handle's scratch)
MATCHING = 0.2  # on the partial cut: at least this share of an unusable field's blocks lies below thsad
CALL3, CALL4, CALL5 = ("U", "S", "E", "V", "S2"), ("S",), ("V", "U")
STANDARD = [(("U",), 0), ((), 0), (CALL3, 0), (CALL4, 0), (CALL5, 0), (("U",), 0), (CALL3, 1), (CALL4, 2), (CALL5, 1)]
# behind every script: a usable and an unusable job change places inside a launch that fits the capacity (call 5 swaps two usable jobs, which a
# usable pass that skipped its store for unusable jobs would survive)
SWAP = [(("U", "S"), 0), (("S", "U"), 0), (("S2", "V", "S"), 0)]


def _oracle():
    import mvoracle
    mvoracle.lib()
    return mvoracle


class World:
    """the clip of one shape and format with everything the oracle derives from it once: super frames and the delta-1 vectors of every frame"""

    def __init__(self, shape, fmt, cut="noise"):
        mo = _oracle()
        self.shape, self.fmt, self.cut = shape, fmt, cut
        self.w, self.h, self.bits, self.akw = SHAPES[shape]
        self.skw = FORMATS[fmt]
        sub = self.skw.get("subsampling", (1, 1))
        frames = pl.moving_clip(self.w, self.h, self.bits, NFRAMES, seed=71, noise=3, sub=sub)
        rng = np.random.default_rng(72)
        for p in frames[CUT]:
            rows = p.shape[0] if cut == "noise" else p.shape[0] * 5 // 8  # "partial": the rows below keep the clip's picture
            p[:rows] = rng.integers(0, 1 << self.bits, (rows, p.shape[1])).astype(p.dtype)
        self.frames = [[f[0]] for f in frames] if self.skw.get("gray") else frames
        self.nplanes = len(self.frames[0])
        self.osup = mo.Super(self.w, self.h, self.bits, **self.skw)
        self.osf = [self.osup.frame(f) for f in self.frames]
        self.oan = {isb: mo.Analyse(self.osup, num_frames=NFRAMES, isb=isb, **self.akw) for isb in (1, 0)}
        self.oan_d = {(isb, 1): self.oan[isb] for isb in (1, 0)}
        self.ad = self.oan[1].ad
        self._blobs, self._finest, self._gpu, self._float = {}, {}, None, None

    @staticmethod
    def nref(t, isb, d=1):
        n = t + d if isb else t - d
        return n if 0 <= n < NFRAMES else None

    def blob(self, t, isb, d=1):
        """vectors of frame t towards its neighbour at distance d (isb: a later frame); the invalid blob when that lies outside the clip"""
        if (t, isb, d) not in self._blobs:
            if (isb, d) not in self.oan_d:
                self.oan_d[isb, d] = _oracle().Analyse(self.osup, num_frames=NFRAMES, isb=isb, delta=d, **self.akw)
            n = self.nref(t, isb, d)
            self._blobs[t, isb, d] = self.oan_d[isb, d].frame(self.osf[t], self.osf[n] if n is not None else None)
        return self._blobs[t, isb, d]

    def pair_blob(self, src, ref):
        assert ref is None or abs(ref - src) == 1
        return self.blob(src, 1 if ref is None or ref > src else 0)

    def usable(self, blob, ad=None, thscd1=400, thscd2=130):
        """the scene-change decision of every vector-consuming filter (MVClip: usable = valid and not a scene change), from the oracle"""
        mo = _oracle()
        a = mo.AnalysisData.from_buffer_copy(bytes(ad if ad is not None else self.ad))
        _, s1, s2 = vector_fields.scaled_thresholds(a, 400, thscd1, thscd2)
        b = np.ascontiguousarray(blob)
        return bool(mo.lib().mvo_blob_is_usable(C.byref(a), C.c_void_p(b.ctypes.data), C.c_int64(s1), C.c_int(s2)))

    def below_thsad(self, blob, thsad, ad=None):
        """share of the blocks whose SAD is below a filter's scaled thsad: the blocks that it compensates"""
        a = ad if ad is not None else self.ad
        return float((pl.blob_vectors(blob, a)[2] < vector_fields.scaled_thresholds(a, thsad)[0]).mean())

    def finest(self, k):
        """mv.Finest of frame k's super frame (what the Flow restatements fetch from)"""
        if k not in self._finest:
            self._finest[k] = self.osup.finest(self.osf[k])
        return self._finest[k]

    def floats(self):
        """(the float clip whose quantised copy is this clip, its float super frames by tests/super_float_ref.py): what the float engines
        read, while their vectors come from the search on the integer clip"""
        if self._float is None:
            import degrain_float_cases as fc
            import super_float_ref
            s = self.osup.s
            ff = fc.float_clip(self.frames, self.bits, seed=9)
            kw = dict(sub=self.skw.get("subsampling", (1, 1)), gray=bool(self.skw.get("gray")), hpad=s.hpad, vpad=s.vpad, pel=s.pel, sharp=s.sharp)
            self._float = (ff, [super_float_ref.frame(f, **kw)[0] for f in ff])
        return self._float

    def gpu_float(self, mv):
        g = self.gpu(mv)
        if not hasattr(g, "fsup"):
            ff, fsf = self.floats()
            g.fsup = mv.Super(self.w, self.h, 32, sample_float=True, **self.skw)
            g.fsrc = [mv.frame_to_device(f) for f in ff]
            g.fsf = [g.fsup.from_host(sf) for sf in fsf]
        return g

    def gpu(self, mv):
        """device copies, made once: the clip, the ORACLE's super frames in the product's layout, and blobs on request"""
        if self._gpu is None:
            g = self._gpu = type("Gpu", (), {})()
            g.sup = mv.Super(self.w, self.h, self.bits, **self.skw)
            g.src = [mv.frame_to_device(f) for f in self.frames]
            g.sf = [g.sup.from_host(sf) for sf in self.osf]
            g.blobs = {}
        return self._gpu

    def gblob(self, mv, host_blob):
        import torch
        g = self.gpu(mv)
        key = id(host_blob)
        if key not in g.blobs:
            g.blobs[key] = (host_blob, torch.from_numpy(host_blob).cuda())  # (the host array is kept: its id is the key)
        return g.blobs[key][1]


@functools.lru_cache(maxsize=None)
def world(shape, fmt="420", cut="noise"):
    return World(shape, fmt, cut)


class Adapter:
    """one handle type with its arguments: makes the handle, runs job descriptors through the Python wrapper, knows the oracle's answer.
    The adapters are module-level objects on purpose: what one keeps across tests is derived from its arguments alone and never changes once
    computed -- the expected outputs per job (_want; the CPU and the GPU tests of a process share them), the restatement objects, device
    copies of the inputs.  What belongs to one run of a script (the blobs kept for prefills, the script's stream) is set anew by make()"""
    nfields = 1           # vector fields per job
    extra_calls = []      # filter-specific calls behind the standard script
    writes_planes = None  # planes the handle writes (None: all)

    def __init__(self, name, shape, fmt="420", **kw):
        self.name, self.shape, self.fmt, self.kw = name, shape, fmt, kw
        self.cut = self.kw.pop("_cut", "noise")
        self._want = {}

    @property
    def world(self):
        return world(self.shape, self.fmt, self.cut) if self.shape is not None else None

    def script(self):
        return STANDARD + list(self.extra_calls) + SWAP

    def expect(self, letter):
        if letter not in self._want:
            self._want[letter] = self._expect(self.jobs[letter])
        return self._want[letter]

    def planes_to_numpy(self, mv, out, want):
        return [mv.plane_to_numpy(out[p], want[p].shape[1], want[p].dtype) for p in range(len(want))]

    # -- what test_handle_sequences.py asks
    def fields(self, letter):
        """[(blob, reference present)] per vector field of the job"""
        raise NotImplementedError

    def extra_fields(self, letter):
        """further fields that a job reads where they are usable (the Flow filters' second pair of vectors)"""
        return []

    def field_ad(self):
        return self.world.ad

    partial = False           # True: no job has all its references usable
    vectors = True            # False: the jobs are not made of vector fields (the Depan warps: transforms), nothing is usable or not
    alike = ()                # jobs whose outputs may be the same by the filter's definition
    s2_one_direction = False  # True: S2 is unusable in exactly one of its fields; False: it is a second job that is unusable in all
    thsad = None          # the thsad under which a block is compensated (None: the filter has none)


class AnalyseAdapter(Adapter):
    """mv.Analyse: jobs (source frame, reference frame or None); every call's destination blobs arrive pre-filled with blobs that an
    earlier call wrote for OTHER jobs, so that the read-back of the coarse levels' predictors cannot lean on leftovers"""
    jobs = {"U": (2, 3), "V": (7, 8), "S": (4, 5), "E": (9, None), "S2": (5, 6)}
    # The handle rotates through KSLOTS job tables, one per call that has jobs.  The standard script's eight such calls give every table the
    # same count twice; these five shift the rotation by one, so that each table is also used with fewer jobs or grown past its headroom
    # (jobs per table over the whole script: 1 1 2 5 | 5 5 1 | 1 1 5 | 2 2 1)
    extra_calls = [(("V", "U"), 0), (("U",), 0), (CALL3, 0), (("S",), 0), (CALL3, 0)]

    def make(self, mv):
        import torch
        self.stale, self.main = [], torch.cuda.current_stream()
        return mv.Analyse(self.world.gpu(mv).sup, num_frames=NFRAMES, isb=1, **self.world.akw)

    def _expect(self, job):
        return [self.world.pair_blob(*job)]

    def _keep(self, letters, out):
        """blobs for later prefills: only those of calls on the script's own stream, which the driver has waited for -- a call on another
        stream then copies finished blobs, whichever stream wrote the call before it"""
        import torch
        if torch.cuda.current_stream() == self.main:
            self.stale = (self.stale + list(zip(letters, out)))[-8:]

    def _prefilled(self, h, letters):
        blobs = h.alloc_blobs(len(letters)) if letters else []
        for i, l in enumerate(letters):
            other = [b for (sl, b) in self.stale if sl != l]
            if other:
                blobs[i].copy_(other[-1])
        return blobs

    def run(self, mv, h, letters):
        g = self.world.gpu(mv)
        jobs = [(g.sf[s], g.sf[r] if r is not None else None) for s, r in (self.jobs[l] for l in letters)]
        out = h.run(jobs, blobs=self._prefilled(h, letters))
        self._keep(letters, out)
        return out

    def to_numpy(self, mv, out, want):
        return [out.cpu().numpy()]

    def fields(self, letter):
        s, r = self.jobs[letter]
        return [(self.world.pair_blob(s, r), r is not None)]


class RecalculateAdapter(AnalyseAdapter):
    """mv.Recalculate on the oracle's delta-1 vectors (one job table, no rotation)"""
    extra_calls = []

    def make(self, mv):
        import torch
        self.stale, self.main = [], torch.cuda.current_stream()
        return mv.Recalculate(self.world.gpu(mv).sup, self.world.ad, **self.kw)

    @functools.lru_cache(maxsize=None)
    def _orc(self):
        return _oracle().Recalculate(self.world.osup, self.world.ad, **self.kw)

    def _expect(self, job):
        s, r = job
        w = self.world
        return [self._orc().frame(w.osf[s], w.osf[r] if r is not None else None, w.pair_blob(s, r))]

    def _prefilled(self, h, letters):
        import torch
        blobs = [torch.zeros(h.blob_size, dtype=torch.uint8, device="cuda") for _ in letters]
        for i, l in enumerate(letters):
            other = [b for (sl, b) in self.stale if sl != l]
            if other:
                blobs[i].copy_(other[-1])
        return blobs

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu(mv)
        jobs = [(g.sf[s], g.sf[r] if r is not None else None, w.gblob(mv, w.pair_blob(s, r))) for s, r in (self.jobs[l] for l in letters)]
        out = h.run(jobs, blobs=self._prefilled(h, letters))
        self._keep(letters, out)
        return out

    def fields(self, letter):
        s, r = self.jobs[letter]
        return [(self.expect(letter)[0], r is not None)]

    def field_ad(self):
        return self._orc().ad


class ScaleVectAdapter(AnalyseAdapter):
    """mv.ScaleVect at scale 2 against tests/scale_vect_ref.py: the jobs are Analyse's blobs, scaled for a super clip of twice the size; M1 and
    M2 are radius-2 multi blobs (fields mvbw, mvfw, mvbw2, mvfw2 of frames 2 and 7 at a stride of whole 256 bytes, zeros between the fields),
    which a call scales with fields=4.  The extra calls alternate the two forms on the one handle"""
    jobs = dict(AnalyseAdapter.jobs, M1=2, M2=7)
    extra_calls = [(("M1",), 0), (("U", "S"), 0), (("M2", "M1"), 0), (("E",), 0), (("M1", "M2"), 0)]
    FIELDS = 4

    @functools.lru_cache(maxsize=None)
    def _target(self):
        """(the super clip of twice the size, the scaled clip's analysis data by the restatement)"""
        import mvtools_amd
        import scale_vect_ref
        w = self.world
        tsup = mvtools_amd.Super(2 * w.w, 2 * w.h, w.bits, **w.skw)
        return tsup, scale_vect_ref.scaled_data(w.ad, 2, tsup.info)

    def make(self, mv):
        return mv.ScaleVect(self.world.ad, self._target()[0], 2)

    def _multi(self, t):
        if ("multi", t) not in self._want:
            blobs = [self.world.blob(t, isb, d) for d in (1, 2) for isb in (1, 0)]
            stride = (blobs[0].size + 255) // 256 * 256
            m = np.zeros(self.FIELDS * stride, np.uint8)
            for r, b in enumerate(blobs):
                m[r * stride:r * stride + b.size] = b
            self._want["multi", t] = (m, stride, (self.FIELDS - 1) * stride + blobs[0].size)
        return self._want["multi", t]

    def _expect(self, job):
        import scale_vect_ref
        w, out_ad = self.world, self._target()[1]
        if isinstance(job, int):
            m, stride, need = self._multi(job)
            return [scale_vect_ref.scale_multi(m, w.ad, out_ad, 2, self.FIELDS, stride)[:need]]
        return [scale_vect_ref.scale_blob(w.pair_blob(*job), w.ad, out_ad, 2)]

    def run(self, mv, h, letters):
        w = self.world
        jobs = [self.jobs[l] for l in letters]
        if not jobs:
            return h.run([], out=[])
        if isinstance(jobs[0], int):
            assert all(isinstance(j, int) for j in jobs), "a call scales single blobs or multi blobs"
            return h.run([w.gblob(mv, self._multi(t)[0]) for t in jobs], fields=self.FIELDS)
        return h.run([w.gblob(mv, w.pair_blob(s, r)) for s, r in jobs])

    def fields(self, letter):
        job = self.jobs[letter]
        if isinstance(job, int):
            return [(self.world.blob(job, isb, d), World.nref(job, isb, d) is not None) for d in (1, 2) for isb in (1, 0)]
        return AnalyseAdapter.fields(self, letter)


class DegrainAdapter(Adapter):
    """mv.Degrain1..6 (radius=): jobs are target frames; the fields are mvbw, mvfw, mvbw2, mvfw2, ...  S2 (frame 4) has the cut behind it
    only, so the count of usable references differs per job inside one launch.  Beyond radius 1 no frame of a ten-frame clip with a cut in
    the middle has all its references: U and V have three or more usable ones, S none, and a launch of five mixes at least three counts"""
    s2_one_direction = True
    jobs = {"U": 2, "V": 7, "S": 5, "E": 0, "S2": 4}
    thsad = 400

    def __init__(self, name, shape, fmt="420", **kw):
        Adapter.__init__(self, name, shape, fmt, **kw)
        self.radius = self.kw.pop("radius", 1)
        self.nfields = 2 * self.radius
        self.partial = self.radius > 1

    def make(self, mv):
        g = self.world.gpu(mv)
        return mv.Degrain(self.radius, g.sup, self.world.ad, [p.stride(0) for p in g.src[0]], **self.kw)

    @property
    def writes_planes(self):
        return [0] if self.kw.get("plane") == 0 else None

    @functools.lru_cache(maxsize=None)
    def _odg(self):
        return _oracle().Degrain(self.radius, self.world.osup, self.world.ad, **self.kw)

    def _order(self):
        return [(isb, d) for d in range(1, self.radius + 1) for isb in (1, 0)]

    def _refs(self, t):
        return [World.nref(t, isb, d) for isb, d in self._order()]

    def _blobs(self, t):
        return [self.world.blob(t, isb, d) for isb, d in self._order()]

    def _expect(self, t):
        w = self.world
        return self._odg().frame(w.frames[t], [w.osf[n] if n is not None else None for n in self._refs(t)], self._blobs(t))

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu(mv)
        jobs = [(g.src[t], [g.sf[n] if n is not None else None for n in self._refs(t)], [w.gblob(mv, b) for b in self._blobs(t)])
                for t in (self.jobs[l] for l in letters)]
        return h.run(jobs, out=None if jobs else [])

    to_numpy = Adapter.planes_to_numpy

    def fields(self, letter):
        t = self.jobs[letter]
        return [(b, n is not None) for b, n in zip(self._blobs(t), self._refs(t))]


class DegrainNAdapter(DegrainAdapter):
    """mv.DegrainN at a radius beyond Degrain's six against tests/degrain_n_ref.py, with the thresholds per distance of degrain_n_cases.tables"""

    def make(self, mv):
        g = self.world.gpu(mv)
        return mv.DegrainN(self.radius, g.sup, self.world.ad, [p.stride(0) for p in g.src[0]], **self.kw)

    def _expect(self, t):
        import degrain_n_cases as dc
        w = self.world
        ref = dc.restatement(_oracle(), self.radius, w.ad, *dc.tables(w.ad, self.radius, self.kw), self.kw, gray=w.fmt == "gray")
        return ref.frame(w.frames[t], [w.osf[n] if n is not None else None for n in self._refs(t)], self._blobs(t))


class CompensateAdapter(Adapter):
    """mv.Compensate (backward vectors): jobs (source frame, reference frame or None)"""
    jobs = AnalyseAdapter.jobs

    def __init__(self, name, shape, fmt="420", **kw):
        Adapter.__init__(self, name, shape, fmt, **kw)
        self.thsad = kw.get("thsad", 10000)

    def make(self, mv):
        return mv.Compensate(self.world.gpu(mv).sup, self.world.ad, **self.kw)

    @functools.lru_cache(maxsize=None)
    def _oc(self):
        return _oracle().Compensate(self.world.osup, self.world.ad, **self.kw)

    def _expect(self, job):
        s, r = job
        w = self.world
        return self._oc().frame(w.osf[s], w.osf[r] if r is not None else None, w.pair_blob(s, r))

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu(mv)
        jobs = [(g.sf[s], g.sf[r] if r is not None else None, w.gblob(mv, w.pair_blob(s, r))) for s, r in (self.jobs[l] for l in letters)]
        return h.run(jobs, out=None if jobs else [])

    to_numpy = Adapter.planes_to_numpy

    def fields(self, letter):
        s, r = self.jobs[letter]
        return [(self.world.pair_blob(s, r), r is not None)]


class CompensateNAdapter(DegrainAdapter):
    """mv.CompensateN at tr 2: a job is a target frame with its multi blob (fields mvbw, mvfw, mvbw2, mvfw2 at a stride of whole 256 bytes) and
    writes the five frames t - 2 .. t + 2 compensated onto t, each what the oracle's Compensate gives for that pair, the clip frame in the middle"""

    def __init__(self, name, shape, fmt="420", **kw):
        DegrainAdapter.__init__(self, name, shape, fmt, radius=2, **kw)
        self.thsad = kw.get("thsad", 10000)

    def make(self, mv):
        h = mv.CompensateN(self.radius, self.world.gpu(mv).sup, self.world.ad, **self.kw)
        assert [h.map(k) for k in range(2 * self.radius + 1)] == self._outputs()
        return h

    def _outputs(self):
        """(offset from the target, field) per output, in temporal order"""
        return [(off, -1 if off == 0 else 2 * (abs(off) - 1) + (0 if off > 0 else 1)) for off in range(-self.radius, self.radius + 1)]

    @functools.lru_cache(maxsize=None)
    def _oc(self, isb, d):
        w = self.world
        w.blob(0, isb, d)  # (makes the oracle's Analyse of this field)
        return _oracle().Compensate(w.osup, w.oan_d[isb, d].ad, **self.kw)

    def _expect(self, t):
        w, out = self.world, []
        for off, field in self._outputs():
            if field < 0:
                out += [p.copy() for p in w.frames[t]]
                continue
            isb, d = self._order()[field]
            n = World.nref(t, isb, d)
            out += self._oc(isb, d).frame(w.osf[t], w.osf[n] if n is not None else None, w.blob(t, isb, d))
        return out

    def _multi(self, mv, t):
        import torch
        g = self.world.gpu(mv)
        if ("multi", t) not in g.blobs:
            blobs = self._blobs(t)
            stride = (blobs[0].size + 255) // 256 * 256
            m = np.zeros(len(blobs) * stride, np.uint8)
            for r, b in enumerate(blobs):
                m[r * stride:r * stride + b.size] = b
            g.blobs["multi", t] = (m, torch.from_numpy(m).cuda())
        return g.blobs["multi", t][1]

    def run(self, mv, h, letters):
        g = self.world.gpu(mv)
        jobs = [(g.sf[t], [g.sf[n] if n is not None else None for n in self._refs(t)], self._multi(mv, t)) for t in (self.jobs[l] for l in letters)]
        return h.run(jobs, out=None if jobs else [])

    def to_numpy(self, mv, out, want):
        flat = [p for fr in out for p in fr]
        return [mv.plane_to_numpy(flat[i], want[i].shape[1], want[i].dtype) for i in range(len(want))]


class DegrainOut16Adapter(DegrainNAdapter):
    """mv.DegrainN with out16 on an 8-bit clip against tests/degrain_out16_ref.py"""

    def make(self, mv):
        g = self.world.gpu(mv)
        return mv.DegrainN(self.radius, g.sup, self.world.ad, [p.stride(0) for p in g.src[0]], out16=True, **self.kw)

    def _expect(self, t):
        import degrain_n_cases as dc
        import degrain_out16_ref as o16
        w = self.world
        ref = o16.restatement(_oracle(), self.radius, w.ad, *dc.tables(w.ad, self.radius, self.kw), self.kw, gray=w.fmt == "gray")
        return o16.frame(ref, w.frames[t], [w.osf[n] if n is not None else None for n in self._refs(t)], self._blobs(t))


class DegrainFloatAdapter(DegrainNAdapter):
    """mv.DegrainN on the float clip (float super frames of the restatement, the integer clip's vectors) against tests/degrain_float_ref.py,
    float32 sample for sample"""

    def make(self, mv):
        g = self.world.gpu_float(mv)
        return mv.DegrainN(self.radius, g.fsup, self.world.ad, [p.stride(0) for p in g.fsrc[0]], **self.kw)

    def _expect(self, t):
        import degrain_float_cases as fc
        import degrain_n_cases as dc
        w = self.world
        ff, fsf = w.floats()
        ref = fc.restatement(_oracle(), self.radius, w.ad, *dc.tables(w.ad, self.radius, self.kw), self.kw, gray=w.fmt == "gray")
        return ref.frame(ff[t], [fsf[n] if n is not None else None for n in self._refs(t)], self._blobs(t))

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu_float(mv)
        jobs = [(g.fsrc[t], [g.fsf[n] if n is not None else None for n in self._refs(t)], [w.gblob(mv, b) for b in self._blobs(t)])
                for t in (self.jobs[l] for l in letters)]
        return h.run(jobs, out=None if jobs else [])


class AnalyseNAdapter(CompensateNAdapter):
    """mv.AnalyseN at radius 2: a job is a target frame with its four references; field r of its multi blob must be the oracle's Analyse(isb,
    delta) blob of that pair.  As for Analyse, the destinations arrive filled with multi blobs that an earlier call wrote for other jobs"""

    def __init__(self, name, shape, fmt="420", **kw):
        CompensateNAdapter.__init__(self, name, shape, fmt, **kw)
        self.thsad = 400

    def make(self, mv):
        import torch
        self.stale, self.main = [], torch.cuda.current_stream()
        h = mv.AnalyseN(self.world.gpu(mv).sup, self.radius, num_frames=NFRAMES, **self.world.akw)
        self.layout = (h.field_stride, h.field_size)
        for r, (isb, d) in enumerate(self._order()):
            self.world.blob(0, isb, d)
            assert bytes(h.ad(r)) == bytes(self._ad(r)), "analysis data of field %d" % r
        return h

    def _ad(self, r):
        return self.world.oan_d[self._order()[r]].ad

    def _expect(self, t):
        return self._blobs(t)

    def _prefilled(self, h, letters):
        blobs = h.alloc_blobs(len(letters)) if letters else []
        for i, l in enumerate(letters):
            other = [b for (sl, b) in self.stale if sl != l]
            if other:
                blobs[i].copy_(other[-1])
        return blobs

    def _jobs(self, mv, letters):
        g = self.world.gpu(mv)
        return [(g.sf[t], [g.sf[n] if n is not None else None for n in self._refs(t)]) for t in (self.jobs[l] for l in letters)]

    def run(self, mv, h, letters):
        import torch
        out = h.run(self._jobs(mv, letters), blobs=self._prefilled(h, letters))
        if torch.cuda.current_stream() == self.main:
            self.stale = (self.stale + list(zip(letters, out)))[-8:]
        return out

    def to_numpy(self, mv, out, want):
        stride, size = self.layout
        a = out.cpu().numpy()
        return [a[r * stride:r * stride + size] for r in range(len(want))]


class RecalculateNAdapter(AnalyseNAdapter):
    """mv.RecalculateN at radius 2 on the oracle's multi blobs: field r must be the oracle's Recalculate of field r"""

    def __init__(self, name, shape, fmt="420", **kw):
        AnalyseNAdapter.__init__(self, name, shape, fmt)
        self.kw = kw

    def make(self, mv):
        import torch
        self.stale, self.main = [], torch.cuda.current_stream()
        self.world.blob(0, 1, 1)
        h = mv.RecalculateN(self.world.gpu(mv).sup, self.world.ad, self.radius, **self.kw)
        self.layout = (h.field_stride, h.field_size)
        return h

    @functools.lru_cache(maxsize=None)
    def _orc(self, isb, d):
        w = self.world
        w.blob(0, isb, d)
        return _oracle().Recalculate(w.osup, w.oan_d[isb, d].ad, **self.kw)

    def _expect(self, t):
        w = self.world
        return [self._orc(isb, d).frame(w.osf[t], w.osf[n] if n is not None else None, w.blob(t, isb, d))
                for (isb, d), n in zip(self._order(), self._refs(t))]

    def _jobs(self, mv, letters):
        return [(s, refs, self._multi(mv, t)) for (s, refs), t in zip(AnalyseNAdapter._jobs(self, mv, letters), (self.jobs[l] for l in letters))]


def float_planes(mv, out, want):
    """float32 output planes (float or byte tensors) as numpy, cut to the reference's widths"""
    import torch
    return [mv.plane_to_numpy(t if t.dtype == torch.uint8 else t.view(torch.uint8), want[i].shape[1], np.float32) for i, t in enumerate(out)]


class CompensateFloatAdapter(CompensateAdapter):
    """mv.Compensate with sample_float=True: the float clip's super frames, the integer clip's vectors, against tests/compensate_float_ref.py"""

    def make(self, mv):
        return mv.Compensate(self.world.gpu_float(mv).fsup, self.world.ad, sample_float=True, **self.kw)

    @functools.lru_cache(maxsize=None)
    def _ref(self):
        import compensate_float_cases as cc
        return cc.restatement(_oracle(), self.world.ad, self.kw, gray=self.world.fmt == "gray")

    def _expect(self, job):
        s, r = job
        fsf = self.world.floats()[1]
        return self._ref().field(fsf[s], fsf[r] if r is not None else None, self.world.pair_blob(s, r))

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu_float(mv)
        jobs = [(g.fsf[s], g.fsf[r] if r is not None else None, w.gblob(mv, w.pair_blob(s, r))) for s, r in (self.jobs[l] for l in letters)]
        return h.run(jobs, out=None if jobs else [])

    def to_numpy(self, mv, out, want):
        return float_planes(mv, out, want)


class CompensateNFloatAdapter(CompensateNAdapter):
    """mv.CompensateN with sample_float=True at tr 2 against compensate_float_ref's job"""

    def make(self, mv):
        h = mv.CompensateN(self.radius, self.world.gpu_float(mv).fsup, self.world.ad, sample_float=True, **self.kw)
        assert [h.map(k) for k in range(2 * self.radius + 1)] == self._outputs()
        return h

    def _expect(self, t):
        import compensate_float_cases as cc
        w = self.world
        fsf = w.floats()[1]
        ref = cc.restatement(_oracle(), w.ad, self.kw, gray=w.fmt == "gray")
        frames = ref.job(self.radius, fsf[t], [fsf[n] if n is not None else None for n in self._refs(t)], self._blobs(t))
        return [p for fr in frames for p in fr]

    def run(self, mv, h, letters):
        g = self.world.gpu_float(mv)
        jobs = [(g.fsf[t], [g.fsf[n] if n is not None else None for n in self._refs(t)], self._multi(mv, t)) for t in (self.jobs[l] for l in letters)]
        return h.run(jobs, out=None if jobs else [])

    def to_numpy(self, mv, out, want):
        return float_planes(mv, [p for fr in out for p in fr], want)


class BlockFPSAdapter(Adapter):
    """mv.BlockFPS at 512 times the rate: jobs are output frames; 512 k is input frame k (time256 0), 512 k + 256 lies half-way (time256 128)
    between k and k + 1, and 512 k + 511 rounds to time256 256, the copy of frame k + 1 (MVBlockFPS.c: time256 = (int)(fraction * 256 + 0.5)
    -- the only way to 256 is a fraction of 511 / 512 and more, hence the rate).  The two vector fields of a job (mvbw of k, mvfw of k + 1)
    are usable or not together: S2 is a second unusable job, on the frames behind the cut.  T0 and T256 are the copy jobs, which the standard
    script's jobs (all half-way) do not have; the extra calls mix them with U and S in one launch"""
    nfields = 2
    RATE = 512
    jobs = {"U": 2 * RATE + 256, "V": 7 * RATE + 256, "S": 4 * RATE + 256, "E": 9 * RATE + 256, "S2": 5 * RATE + 256, "T0": 6 * RATE, "T256": 2 * RATE + 511}
    extra_calls = [(("T0", "U", "S", "T256"), 0), (("S", "T256", "T0"), 0)]

    def make(self, mv):
        g = self.world.gpu(mv)
        return mv.BlockFPS(g.sup, self.world.ad, self.world.oan[0].ad, NFRAMES, [p.stride(0) for p in g.src[0]], 24, 1, num=24 * self.RATE, den=1, **self.kw)

    @functools.lru_cache(maxsize=None)
    def _ob(self):
        return _oracle().BlockFPS(self.world.osup, self.world.ad, self.world.oan[0].ad, NFRAMES, 24, 1, num=24 * self.RATE, den=1, **self.kw)

    def _clips(self):
        w = self.world
        return [w.blob(n, 1) for n in range(NFRAMES)], [w.blob(n, 0) for n in range(NFRAMES)]

    def _expect(self, n):
        w = self.world
        bw, fw = self._clips()
        return self._ob().frame(n, w.frames, w.osf, bw, fw)

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu(mv)
        bw, fw = self._clips()
        ns = [self.jobs[l] for l in letters]
        return h.run(ns, g.src, g.sf, [w.gblob(mv, b) for b in bw], [w.gblob(mv, b) for b in fw], out=None if ns else [])

    to_numpy = Adapter.planes_to_numpy

    def fields(self, letter):
        nl, nr, _ = self._ob().map(self.jobs[letter])
        good = nl < NFRAMES and nr < NFRAMES
        w = self.world
        return [(w.blob(min(nl, NFRAMES - 1), 1), good), (w.blob(min(nr, NFRAMES - 1), 0), good)]


class BlockFPSFloatAdapter(BlockFPSAdapter):
    """mv.BlockFPS with sample_float=True against tests/blockfps_float_ref.py: the float clip and its super frames, the integer clip's vectors"""

    def make(self, mv):
        g = self.world.gpu_float(mv)
        return mv.BlockFPS(g.fsup, self.world.ad, self.world.oan[0].ad, NFRAMES, [p.stride(0) for p in g.fsrc[0]], 24, 1, num=24 * self.RATE, den=1,
                           sample_float=True, **self.kw)

    def _expect(self, n):
        import blockfps_float_cases as bc
        w = self.world
        ff, fsf = w.floats()
        bw, fw = self._clips()
        ref = bc.restatement(_oracle(), w.ad, w.oan[0].ad, self.kw, gray=w.fmt == "gray")
        return bc.want_frame(ref, self._ob().map, n, ff, fsf, bw, fw)

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu_float(mv)
        bw, fw = self._clips()
        ns = [self.jobs[l] for l in letters]
        return h.run(ns, g.fsrc, g.fsf, [w.gblob(mv, b) for b in bw], [w.gblob(mv, b) for b in fw], out=None if ns else [])

    def to_numpy(self, mv, out, want):
        return float_planes(mv, out, want)


class FlowAdapter(Adapter):
    """mv.FlowFPS (24 -> 60: five outputs per two inputs, time256 0, 102, 205, 51, 154) and, with time=, mv.FlowInter (output n lies between
    n and n + 1) against tests/flow_ref.py.  A job's main fields are mvbw of its left and mvfw of its right frame, the extra pair mvfw of the
    left and mvbw of the right one.  FlowFPS has no output behind the last input frame: its E lies between frames 0 and 1, where the extra
    mvfw of frame 0 is the invalid blob."""
    nfields = 2

    def __init__(self, name, shape, fmt="420", **kw):
        Adapter.__init__(self, name, shape, fmt, **kw)
        self.fps = "time" not in kw
        if self.fps:
            self.jobs = {"U": 6, "V": 18, "S": 11, "E": 1, "S2": 14, "T0": 5}
            self.extra_calls = [(("T0", "U", "S", "V"), 0), (("S", "T0"), 0)]
        else:
            self.jobs = {"U": 2, "V": 7, "S": 4, "E": 9, "S2": 5}

    def make(self, mv):
        w, g = self.world, self.world.gpu(mv)
        pitch = [p.stride(0) for p in g.src[0]]
        if self.fps:
            return mv.FlowFPS(g.sup, w.ad, w.oan[0].ad, NFRAMES, pitch, 24, 1, num=60, den=1, **self.kw)
        return mv.FlowInter(g.sup, w.ad, w.oan[0].ad, NFRAMES, pitch, **self.kw)

    @functools.lru_cache(maxsize=None)
    def _ref(self):
        import flow_ref
        w = self.world
        kw = dict(fps=(24, 1), num=60, den=1, **self.kw) if self.fps else self.kw
        return flow_ref.Flow(w.ad, w.oan[0].ad, NFRAMES, w.nplanes, w.osup.s.hpad, w.osup.s.vpad, **kw)

    def _clips(self):
        w = self.world
        return [w.blob(n, 1) for n in range(NFRAMES)], [w.blob(n, 0) for n in range(NFRAMES)]

    def _expect(self, n):
        w = self.world
        bw, fw = self._clips()
        return self._ref().frame(n, w.frames, w.finest, bw, fw)

    def kind(self, letter):
        """the formula or fallback the restatement takes for the job (flow_ref.Flow.last_kind)"""
        self._expect(self.jobs[letter])
        return self._ref().last_kind

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu(mv)
        bw, fw = self._clips()
        ns = [self.jobs[l] for l in letters]
        return h.run(ns, g.src, g.sf, [w.gblob(mv, b) for b in bw], [w.gblob(mv, b) for b in fw], out=None if ns else [])

    to_numpy = Adapter.planes_to_numpy

    def fields(self, letter):
        nl, nr, _ = self._ref().map(self.jobs[letter])
        good = nl < NFRAMES and nr < NFRAMES
        w = self.world
        return [(w.blob(min(nl, NFRAMES - 1), 1), good), (w.blob(min(nr, NFRAMES - 1), 0), good)]

    def extra_fields(self, letter):
        nl, nr, _ = self._ref().map(self.jobs[letter])
        if nr >= NFRAMES:
            return []
        return [(self.world.blob(nl, 0), World.nref(nl, 0) is not None), (self.world.blob(nr, 1), World.nref(nr, 1) is not None)]


class FlowCompAdapter(Adapter):
    """mv.Flow on the backward vectors against tests/flowmc_ref.py: job n is clip frame n compensated from frame n + 1; mode 1 scatters the
    samples through the 64-bit atomicMax window that the handle keeps (dWin).  An unusable job copies its clip frame"""
    jobs = {"U": 2, "V": 7, "S": 4, "E": 9, "S2": 5}

    def make(self, mv):
        w, g = self.world, self.world.gpu(mv)
        return mv.Flow(g.sup, w.ad, NFRAMES, [p.stride(0) for p in g.src[0]], **self.kw)

    @functools.lru_cache(maxsize=None)
    def _ref(self):
        import flowmc_ref
        w = self.world
        return flowmc_ref.Flow(w.ad, NFRAMES, w.nplanes, w.osup.s.hpad, w.osup.s.vpad, w.bits, **self.kw)

    def _expect(self, n):
        w = self.world
        return self._ref().frame(n, w.frames, w.finest, w.blob(n, 1))

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu(mv)
        jobs = [(g.src[n], g.sf[n + 1] if n + 1 < NFRAMES else None, w.gblob(mv, w.blob(n, 1))) for n in (self.jobs[l] for l in letters)]
        return h.run(jobs, out=None if jobs else [])

    to_numpy = Adapter.planes_to_numpy

    def fields(self, letter):
        n = self.jobs[letter]
        return [(self.world.blob(n, 1), n + 1 < NFRAMES)]


class FlowBlurAdapter(Adapter):
    """mv.FlowBlur against tests/flowmc_ref.py: frame n reads mvbw of n - 1 and mvfw of n + 1; frame 4 has the cut on one side only"""
    nfields = 2
    s2_one_direction = True
    jobs = {"U": 2, "V": 7, "S": 5, "E": 0, "S2": 4}

    def make(self, mv):
        w, g = self.world, self.world.gpu(mv)
        return mv.FlowBlur(g.sup, w.ad, w.oan[0].ad, NFRAMES, [p.stride(0) for p in g.src[0]], **self.kw)

    @functools.lru_cache(maxsize=None)
    def _ref(self):
        import flowmc_ref
        w = self.world
        return flowmc_ref.FlowBlur(w.ad, w.oan[0].ad, NFRAMES, w.nplanes, w.osup.s.hpad, w.osup.s.vpad, w.bits, **self.kw)

    def _clips(self):
        w = self.world
        return [w.blob(n, 1) for n in range(NFRAMES)], [w.blob(n, 0) for n in range(NFRAMES)]

    def _expect(self, n):
        w = self.world
        return self._ref().frame(n, w.frames, w.finest, *self._clips())

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu(mv)
        bw, fw = self._clips()
        ns = [self.jobs[l] for l in letters]
        return h.run(ns, g.src, g.sf, [w.gblob(mv, b) for b in bw], [w.gblob(mv, b) for b in fw], out=None if ns else [])

    to_numpy = Adapter.planes_to_numpy

    def fields(self, letter):
        n, w = self.jobs[letter], self.world
        ok = n - 1 >= 0 and n + 1 < NFRAMES
        return [(w.blob(max(n - 1, 0), 1), ok), (w.blob(min(n + 1, NFRAMES - 1), 0), ok)]


class MaskAdapter(Adapter):
    """mv.Mask on the backward vectors against tests/mask_ref.py (deep=True: mask_deep_ref at the clip's depth): jobs are blobs, by (frame,
    its reference).  A frame whose vectors are unusable is filled with ysc, so S, S2 and E give the same planes (kind 5: but for the luma)"""
    jobs = AnalyseAdapter.jobs
    alike = ("S", "S2", "E")

    def __init__(self, name, shape, fmt="420", **kw):
        Adapter.__init__(self, name, shape, fmt, **kw)
        self.deep = self.kw.pop("deep", False)

    def make(self, mv):
        w, g = self.world, self.world.gpu(mv)
        kw = dict(self.kw)
        if self.kw["kind"] == 5:
            kw["clip_pitch"] = [g.src[0][0].stride(0)]
        return mv.Mask(w.ad, w.w, w.h, subsampling=w.skw.get("subsampling", (1, 1)), bits=w.bits if self.deep else 8, deep=self.deep, **kw)

    @functools.lru_cache(maxsize=None)
    def _ref(self):
        import mask_deep_ref
        import mask_ref
        return mask_deep_ref.DeepMask(self.world.ad, self.world.bits, **self.kw) if self.deep else mask_ref.Mask(self.world.ad, **self.kw)

    def _expect(self, job):
        s, r = job
        return self._ref().frame(self.world.pair_blob(s, r), self.world.frames[s][0] if self.kw["kind"] == 5 else None, {})

    def run(self, mv, h, letters):
        w, g = self.world, self.world.gpu(mv)
        jobs = [self.jobs[l] for l in letters]
        clip = [g.src[s] for s, _ in jobs] if self.kw["kind"] == 5 else None
        return h.run([w.gblob(mv, w.pair_blob(s, r)) for s, r in jobs], clip, out=None if jobs else [])

    to_numpy = Adapter.planes_to_numpy

    def fields(self, letter):
        s, r = self.jobs[letter]
        return [(self.world.pair_blob(s, r), r is not None)]


class DepanCompensateAdapter(Adapter):
    """mv.DepanCompensate on a crafted case of tests/depan_cases.py: the jobs are transforms of one noise frame, by index into the case's
    list -- rotations (the longest position chains), zooms and plain shifts, so that the chains of a launch, and of one slot from call to call,
    differ in length (dChain, dPlanes)"""
    vectors = False

    def __init__(self, name, case, jobs):
        import depan_cases
        Adapter.__init__(self, name, None)
        self.case = next(c for c in depan_cases.CASES if c["name"] == case)
        self.jobs = dict(zip(("U", "V", "S", "E", "S2"), jobs))

    def _inputs(self, mv):
        import depan_cases
        if not hasattr(self, "_dev"):
            self._dev = [mv.plane_to_device(p) for p in depan_cases.expected(self.case)[0]]
        return self._dev

    def make(self, mv):
        import depan_cases
        c, f = self.case, depan_cases.FORMATS[self.case["fmt"]]
        return mv.DepanCompensate(c["w"], c["h"], c["bits"], f["subsampling"], f.get("gray", False), src_pitch=[d.stride(0) for d in self._inputs(mv)],
                                  offset=1.0, subpixel=c["sub"], mirror=c["mirror"], blur=c["blur"])

    def _expect(self, k):
        import depan_cases
        return depan_cases.expected(self.case)[1][k]

    def run(self, mv, h, letters):
        ks = [self.jobs[l] for l in letters]
        return h.run([self._inputs(mv)] * len(ks), [self.case["trs"][k] for k in ks], out=None if ks else [])

    to_numpy = Adapter.planes_to_numpy


class DepanStabiliseAdapter(DepanCompensateAdapter):
    """mv.DepanStabilise on the crafted plans of tests/depan_stab_cases.py: a job paints the current frame and fills from the next and the
    previous one where its plan names them, each under a transform of its own"""

    def __init__(self, name, case, jobs):
        import depan_stab_cases
        Adapter.__init__(self, name, None)
        self.case = next(c for c in depan_stab_cases.CASES if c["name"] == case)
        self.jobs = dict(zip(("U", "V", "S", "E", "S2"), jobs))

    def _inputs(self, mv):
        import depan_stab_cases
        if not hasattr(self, "_dev"):
            self._dev = [[mv.plane_to_device(p) for p in fr] for fr in depan_stab_cases.expected(self.case)[0]]
        return self._dev

    def make(self, mv):
        import depan_cases
        c, f = self.case, depan_cases.FORMATS[self.case["fmt"]]
        return mv.DepanStabilise(c["w"], c["h"], c["bits"], f["subsampling"], f.get("gray", False), src_pitch=[d.stride(0) for d in self._inputs(mv)[0]],
                                 subpixel=c["sub"], mirror=c["mirror"], blur=c["blur"], prev=1, next=1, num_frames=3)

    def _expect(self, k):
        import depan_stab_cases
        return depan_stab_cases.expected(self.case)[1][k]

    def _plan(self, mv, cur, nxt, prev):
        p = mv.DepanStabilisePlan()
        p.tr[:] = [float(v) for v in cur]
        for name, src in (("next", nxt), ("prev", prev)):
            if src is not None:
                d = getattr(p, name)
                d.used, d.frame = 1, src[0]
                d.tr[:] = [float(v) for v in src[1]]
        return p

    def run(self, mv, h, letters):
        dev = self._inputs(mv)
        js = [self.case["jobs"][self.jobs[l]] for l in letters]
        n = len(js)
        arr, out = h.jobs([self._plan(mv, *j) for j in js], [dev[0]] * n, [dev[j[2][0]] if j[2] else None for j in js], [dev[j[1][0]] if j[1] else None for j in js],
                          out=None if n else [])
        h.launch(arr)
        return out


class DepanAnalyseAdapter(Adapter):
    """mv.DepanAnalyse against depan_ref.Analyse: jobs are blobs of the backward (isb=1) or forward vectors, with or without a mask clip; the
    result is the motion (dx, dy, zoom, rot, error as float32 bits, and the iteration count).  Unusable vectors give the null motion, so S,
    S2 and E answer alike"""
    alike = ("S", "S2", "E")

    def __init__(self, name, shape, isb, masked):
        Adapter.__init__(self, name, shape)
        self.isb, self.masked = isb, masked
        self.jobs = AnalyseAdapter.jobs if isb else {"U": (3, 2), "V": (8, 7), "S": (5, 4), "E": (0, None), "S2": (6, 5)}

    def field_ad(self):
        return self.world.oan[self.isb].ad

    def _blob(self, job):
        s, r = job
        return self.world.blob(s, self.isb)

    def _mask(self):
        w = self.world
        m = np.random.default_rng(8).integers(0, 256, (w.h, w.w)).astype(np.uint8)
        m[:, 100:] = 255
        return m

    def make(self, mv):
        w = self.world
        if self.masked and not hasattr(self, "_dmask"):
            self._dmask = mv.plane_to_device(self._mask())
        return mv.DepanAnalyse(self.field_ad(), w.w, w.h, bits=w.bits, mask=(8,) if self.masked else None)

    @functools.lru_cache(maxsize=None)
    def _ref(self):
        import depan_ref
        w, ad = self.world, self.field_ad()
        _, s1, s2 = vector_fields.scaled_thresholds(ad, 400)
        return depan_ref.Analyse(ad, w.w, w.h, s1, s2, has_mask=self.masked)

    @staticmethod
    def _arrays(m):
        return [np.append(np.array([m[k] for k in ("dx", "dy", "zoom", "rot", "error")], np.float32).view(np.uint32), np.uint32(m["iter"]))]

    def _expect(self, job):
        return self._arrays(self._ref().frame(self._blob(job), self._mask() if self.masked else None))

    def run(self, mv, h, letters):
        blobs = [self.world.gblob(mv, self._blob(self.jobs[l])) for l in letters]
        return h.run(blobs, [self._dmask] * len(blobs) if self.masked and blobs else None)  # (the wrapper takes the pitch from the first mask)

    def to_numpy(self, mv, out, want):
        return self._arrays(out)

    def fields(self, letter):
        return [(self._blob(self.jobs[letter]), self.jobs[letter][1] is not None)]


A8, B16, C8 = "8bit-blk8-ov4", "16bit-blk16-ov8", "8bit-blk8-ov0"

ADAPTERS = [
    AnalyseAdapter("analyse-8bit", A8),      # a launch of up to 5 chains: the team form
    AnalyseAdapter("analyse-16bit", B16),
    AnalyseAdapter("analyse-8bit-ov0", C8),
    RecalculateAdapter("recalculate-8bit", A8, blksize=16, overlap=8, thsad=80),
    RecalculateAdapter("recalculate-16bit", B16, blksize=8, overlap=4, thsad=100),
    DegrainAdapter("degrain1-8bit", A8),
    DegrainAdapter("degrain1-16bit", B16),
    DegrainAdapter("degrain1-8bit-ov0", C8),
    DegrainAdapter("degrain1-8bit-luma", A8, plane=0),
    DegrainAdapter("degrain1-8bit-444", A8, "444"),
    DegrainAdapter("degrain1-8bit-gray", A8, "gray"),
    DegrainAdapter("degrain3-8bit", A8, radius=3),
    DegrainAdapter("degrain3-16bit", B16, radius=3),       # six references: the plan tile of the cell kernel
    DegrainAdapter("degrain3-8bit-ov0", C8, radius=3),
    DegrainNAdapter("degrain8-8bit", A8, radius=8),
    DegrainNAdapter("degrain8-16bit", B16, radius=8),
    DegrainNAdapter("degrain8-8bit-ov0-luma", C8, radius=8, plane=0),
    DegrainNAdapter("degrain8-8bit-gray", A8, "gray", radius=8),
    DegrainOut16Adapter("degrain8-out16", A8, radius=8),
    DegrainOut16Adapter("degrain3-out16-ov0", C8, radius=3, limit=3000, limitc=5000),
    DegrainFloatAdapter("degrain8-float-8bit-vectors", A8, radius=8),
    DegrainFloatAdapter("degrain3-float-16bit-vectors", B16, radius=3),
    DegrainFloatAdapter("degrain3-float-ov0-luma", C8, radius=3, plane=0),
    # Across a cut to pure noise every block's SAD is far above thsad, its weight is 0 with or without the usable flag, and a Degrain that took
    # a stale flag for S would still be right.  On the partial cut (noise in the upper five eighths of frame 5) S is a scene change whose lower
    # blocks match: taken for usable they would be blended in
    DegrainAdapter("degrain1-8bit-partial-cut", A8, _cut="partial"),
    DegrainAdapter("degrain1-16bit-partial-cut", B16, _cut="partial"),
    CompensateAdapter("compensate-8bit-sc1", A8, scbehavior=1),
    CompensateAdapter("compensate-8bit-sc0", A8, scbehavior=0),
    CompensateAdapter("compensate-16bit-sc0", B16, scbehavior=0),
    CompensateAdapter("compensate-8bit-ov0-sc0", C8, scbehavior=0),
    CompensateAdapter("compensate-8bit-thsad", A8, scbehavior=0, thsad=150),  # low enough that some blocks of U and V fall back on the source
    CompensateAdapter("compensate-8bit-444", A8, "444", scbehavior=0),
    CompensateAdapter("compensate-8bit-gray", A8, "gray", scbehavior=0),
    CompensateNAdapter("compensate2-8bit-sc0", A8, scbehavior=0),
    CompensateNAdapter("compensate2-16bit-sc1-thsad", B16, scbehavior=1, thsad=150),
    CompensateNAdapter("compensate2-8bit-ov0-sc0", C8, scbehavior=0),
    CompensateFloatAdapter("compensate-float-sc0", A8, scbehavior=0),
    CompensateFloatAdapter("compensate-float-16bit-vectors-sc1-thsad", B16, scbehavior=1, thsad=150),
    CompensateFloatAdapter("compensate-float-ov0-sc0", C8, scbehavior=0),
    CompensateNFloatAdapter("compensate2-float-sc0", A8, scbehavior=0),
    CompensateNFloatAdapter("compensate2-float-16bit-vectors-sc1", B16, scbehavior=1),
    AnalyseNAdapter("analyse2-8bit", A8),
    AnalyseNAdapter("analyse2-16bit", B16),
    RecalculateNAdapter("recalculate2-8bit", A8, blksize=16, overlap=8, thsad=80),
    RecalculateNAdapter("recalculate2-16bit", B16, blksize=8, overlap=4, thsad=100),
] + [BlockFPSAdapter("blockfps-8bit-mode%d" % m, A8, mode=m, **({"ml": 40.0} if m >= 3 else {})) for m in (0, 2, 3, 4, 8)] + [
    BlockFPSAdapter("blockfps-16bit-mode3", B16, mode=3, ml=40.0),
    BlockFPSAdapter("blockfps-8bit-ov0-mode2", C8, mode=2),
    BlockFPSAdapter("blockfps-8bit-mode0-noblend", A8, mode=0, blend=0),
    BlockFPSAdapter("blockfps-8bit-444-mode4", A8, "444", mode=4, ml=40.0),
    BlockFPSAdapter("blockfps-8bit-gray-mode3", A8, "gray", mode=3, ml=40.0),
    BlockFPSFloatAdapter("blockfps-float-mode0", A8, mode=0),
    BlockFPSFloatAdapter("blockfps-float-mode3", A8, mode=3, ml=40.0),
    BlockFPSFloatAdapter("blockfps-float-16bit-vectors-mode4", B16, mode=4, ml=40.0),
    BlockFPSFloatAdapter("blockfps-float-ov0-mode8", C8, mode=8, ml=40.0),
]
ADAPTERS += [FlowAdapter("flowfps-8bit-mask%d" % m, A8, mask=m) for m in (0, 1, 2)] + [
    FlowAdapter("flowfps-16bit-mask2", B16, mask=2, ml=40.0),
    FlowAdapter("flowfps-8bit-ov0-mask2-noblend", C8, mask=2, blend=0),
    FlowAdapter("flowfps-8bit-444-mask2", A8, "444", mask=2),
    FlowAdapter("flowfps-8bit-gray-mask1", A8, "gray", mask=1),
    FlowAdapter("flowinter-8bit-time50", A8, time=50.0),
    FlowAdapter("flowinter-8bit-time33-noblend", A8, time=33.0, blend=0),
    FlowAdapter("flowinter-16bit-time50", B16, time=50.0, ml=40.0),
    FlowAdapter("flowinter-8bit-time0", A8, time=0.0),            # (FlowInter has no copy shortcut: times 0 and 100 run the formulas at time256 0 and 256)
    FlowAdapter("flowinter-8bit-time100", A8, time=100.0),
    FlowAdapter("flowinter-8bit-ov0-time100-noblend", C8, time=100.0, blend=0),
    FlowAdapter("flowinter-8bit-gray-time50", A8, "gray", time=50.0),
    FlowAdapter("flowinter-8bit-444-time0", A8, "444", time=0.0),
]
ADAPTERS += [
    FlowCompAdapter("flow-8bit-fetch", A8, mode=0),
    FlowCompAdapter("flow-8bit-shift", A8, mode=1),
    FlowCompAdapter("flow-16bit-shift-time40", B16, mode=1, time=40.0),
    FlowCompAdapter("flow-8bit-ov0-shift", C8, mode=1),
    FlowCompAdapter("flow-8bit-gray-shift", A8, "gray", mode=1),
    FlowBlurAdapter("flowblur-8bit", A8, blur=50.0, prec=1),
    FlowBlurAdapter("flowblur-16bit", B16, blur=50.0, prec=1),
    FlowBlurAdapter("flowblur-8bit-444", A8, "444", blur=50.0, prec=1),

    MaskAdapter("mask-8bit-kind0", A8, kind=0, ysc=0, ml=10.0),
    MaskAdapter("mask-8bit-kind1-time37", A8, kind=1, time=37.5, ysc=200),
    MaskAdapter("mask-8bit-kind1-time0", A8, kind=1, time=0.0),
    MaskAdapter("mask-8bit-kind2-time37", A8, kind=2, time=37.5, ml=10.0),
    MaskAdapter("mask-8bit-ov0-kind2-time100", C8, kind=2, time=100.0, ysc=200, ml=10.0),
    MaskAdapter("mask-8bit-444-kind2-time0", A8, "444", kind=2, time=0.0, ml=10.0),
    MaskAdapter("mask-8bit-kind3", A8, kind=3, ml=10.0),
    MaskAdapter("mask-8bit-kind4", A8, kind=4, ysc=200, ml=10.0),
    MaskAdapter("mask-8bit-ov0-kind5", C8, kind=5, ml=10.0),
    MaskAdapter("mask-16bit-deep-kind1-time37", B16, kind=1, time=37.5, deep=True),
    MaskAdapter("mask-16bit-deep-kind2-time37", B16, kind=2, time=37.5, ml=10.0, ysc=200, deep=True),
    MaskAdapter("mask-16bit-deep-kind5", B16, kind=5, ml=10.0, deep=True),
]
ADAPTERS += [ScaleVectAdapter("scalevect-8bit", A8), ScaleVectAdapter("scalevect-16bit", B16), ScaleVectAdapter("scalevect-8bit-ov0", C8)]
ADAPTERS += [
    DepanCompensateAdapter("depancompensate-8bit-bilinear", "mirror15_s1", (6, 4, 0, 7, 5)),   # rotation, zoom, shift, rotation, zoom
    DepanCompensateAdapter("depancompensate-8bit-nearest", "mirror15_s0", (0, 6, 4, 1, 7)),
    DepanCompensateAdapter("depancompensate-16bit-bicubic-blur", "blur1_s2", (4, 5, 0, 1, 2)),
    DepanCompensateAdapter("depancompensate-gray-16bit", "gray_s1", (5, 4, 0, 2, 1)),
    DepanStabiliseAdapter("depanstabilise-8bit-bilinear", "combos_s1_8", (1, 0, 5, 9, 3)),      # three rotations; three shifts; no next; the current frame alone; mixed
    DepanStabiliseAdapter("depanstabilise-16bit-bicubic", "combos_s2_16", (2, 4, 7, 10, 6)),
    DepanStabiliseAdapter("depanstabilise-8bit-nearest-mirror", "mirror15_s0", (0, 1, 2, 6, 3)),
]
ADAPTERS += [
    DepanAnalyseAdapter("depananalyse-8bit-backward", A8, 1, False),
    DepanAnalyseAdapter("depananalyse-8bit-forward-masked", A8, 0, True),
    DepanAnalyseAdapter("depananalyse-16bit-backward-masked", B16, 1, True),
    DepanAnalyseAdapter("depananalyse-8bit-ov0-forward", C8, 0, False),
]
BY_NAME = {a.name: a for a in ADAPTERS}


def differing(got, want):
    """'' when every array of the two lists is equal, else which differ"""
    bad = ["output %d: %d of %d values differ" % (i, int(np.count_nonzero(g != w)), w.size) for i, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]
    return "; ".join(bad)


def run_script(mv, adapter, script=None):
    """Runs the script on ONE handle and compares every output of every call bit for bit with the oracle.  On a mismatch the failing call is
    repeated alone on a fresh handle, and the message says whether that agrees with the reference: that tells a stale-scratch bug (agrees)
    from a plain parity bug (does not)."""
    import torch
    script = script if script is not None else adapter.script()
    h = adapter.make(mv)
    torch.cuda.synchronize()
    main = torch.cuda.current_stream()
    side = {1: torch.cuda.Stream(), 2: torch.cuda.Stream()}
    pending, failures = [], []

    def compare(ci, letters, outs):
        for l, out in zip(letters, outs):
            want = adapter.expect(l)
            bad = differing(adapter.to_numpy(mv, out, want), want)
            if bad:
                failures.append((ci, letters, "call %d %s, job %s: %s" % (ci + 1, list(letters), l, bad)))

    for ci, (letters, stream) in enumerate(script):
        if stream == 0:
            outs = adapter.run(mv, h, letters)
            torch.cuda.synchronize()
            assert len(outs) == len(letters)
            compare(ci, letters, outs)      # (copies the outputs away before the next call)
        else:
            s = side[stream]
            s.wait_stream(main)             # the inputs were produced on the caller's stream
            with torch.cuda.stream(s):
                pending.append((ci, letters, adapter.run(mv, h, letters)))  # (destinations of its own; no host synchronisation)
    torch.cuda.synchronize()
    for ci, letters, outs in pending:
        compare(ci, letters, outs)
    if failures:
        msgs = []
        for ci, letters, msg in failures[:6]:
            fresh = adapter.make(mv)
            outs = adapter.run(mv, fresh, letters)
            torch.cuda.synchronize()
            agrees = all(not differing(adapter.to_numpy(mv, o, adapter.expect(l)), adapter.expect(l)) for l, o in zip(letters, outs))
            msgs.append(msg + " -- a fresh handle %s with the reference" % ("agrees" if agrees else "disagrees"))
        raise AssertionError("%s: %d outputs differ from the oracle\n" % (adapter.name, len(failures)) + "\n".join(msgs))
