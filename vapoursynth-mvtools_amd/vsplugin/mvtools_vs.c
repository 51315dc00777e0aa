/*
 * mvtools_vs.c -- VapourSynth API-4 filter shell over libmvtools_amd.so (the C ABI in include/mvtools_amd.h).
 *
 * Registers, under the reference's plugin id / namespace ("com.nodame.mvtools", "mv"), the filters of the hot path
 * with the reference's exact argument strings:
 *     Super       (src/MVSuper.c:279-291)        Analyse   (src/MVAnalyse.c:639-671)
 *     Degrain1..6 (src/MVDegrains.cpp:813-932)   Compensate (src/MVCompensate.c:579-592)   BlockFPS (src/MVBlockFPS.c:1017-1033)
 *     Recalculate (src/MVRecalculate.c:549-572)   Finest (src/MVFinest.c:213-218)   SCDetection (src/MVSCDetection.c:137-145)
 * and, when the host's environment has MVX_VS_FLOW=1 as the plugin is loaded, the per-sample filters
 *     FlowInter (src/MVFlowInter.c:700-710)   FlowFPS (src/MVFlowFPS.c:913-925)   Flow (src/MVFlow.cpp:597-607)
 *     FlowBlur  (src/MVFlowBlur.c:555-565)    Mask    (src/MVMask.c:350-360; with MVX_VS_MASK_DEEP=1 as well: clips of 9 to 16 bits, masks of the clip's depth)
 * and, with MVX_VS_DEPAN=1, the global-motion filters (src/MVDepan.cpp:4211-4288)
 *     DepanAnalyse   DepanEstimate   DepanCompensate   DepanStabilise
 * and, with MVX_VS_MULTI=1, the temporal-radius filters over the multi vector clip (no reference counterpart; see their section)
 *     AnalyseN   RecalculateN   DegrainN   CompensateN   MultiField
 * With MVX_VS_FLOAT=1 mv.Super and the filters that have a float entry in the library take 32-bit float clips; the switch registers no function (see g_vs_float).
 * DepanEstimate is ONE node where the reference chains three: its temporary DepanEstimateFFT / FFT2 and DepanEstimateX / Y / Zoom / Trust frame properties do not
 * exist here (the spectra stay on the device, the stage-2 results in a table of the instance); info=1 sets Depan*_info and invokes text.FrameProps as the reference does.
 * The shell keeps the reference's inter-filter data layout: super-frame geometry + Super_* props on frame 0
 * (src/MVSuper.c:111-120), vector clips = copyFrame(super[n]) + binary props MVTools_MVAnalysisData / MVTools_vectors
 * (src/MVAnalyse.c:224-239).  This file is the only code that touches VSAPI; all arithmetic happens on the GPU behind
 * the C ABI, and every compute failure surfaces through setFilterError (there is no CPU path).
 *
 * Super frames produced here stay resident in a device-side cache (keyed by a per-frame id prop and checked against a
 * fingerprint of the host frame) so that Analyse / Degrain / Compensate do not round-trip 131 MB pyramids through host
 * memory; frames that did not come from this Super, or that another filter modified, are uploaded on demand.
 * mv.Analyse batches: the getFrame calls that VapourSynth's worker threads make concurrently (every filter here is
 * fmParallel, like the reference: MVAnalyse.c:634) are collected by a combining queue into ONE mvx_analyse_frames launch per
 * instance on the instance's own stream -- the search is a serial chain per frame whose throughput comes from the number
 * of chains in flight.  The other filters make one C-ABI call per frame; all handles are thread-safe.
 *
 * dct 1..4 of Analyse / Recalculate (the float block DCT as luma cost) are opt-in: with MVX_VS_DCT=1 in the host's environment as the
 * plugin is loaded the shell calls mvx_enable_dct_float(1) once; without it they fail loudly at creation, like the C ABI's default, and nothing here changes.
 */
#include <errno.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "vs4_api.h"
#include "vs4_api_check.h"
#include "../../include/mvtools_amd.h"
#include "mvx_vs_window.h"

#define PROP_ADATA "MVTools_MVAnalysisData"
#define PROP_VECTORS "MVTools_vectors"
#define PROP_SUPER_ID "_MVX_SuperId"

/* MVX_VS_FLOAT=1 (read once, at the entry point): mv.Super and the filters with a float entry in the library take 32-bit float clips.  It registers no
 * function and changes no argument string; without it every format test and message below is what it was.  A float clip is one the host calls stFloat with 32 bits. */
static int g_vs_float;
static int vi_is_float(const VSVideoInfo *vi) { return g_vs_float && vi->format.sampleType == stFloat && vi->format.bitsPerSample == 32; }
/* the reference's format test of a `super` argument (MVAnalyse.c:506, MVFinest.c:165).  With the switch a float super clip passes it, so that the library's creation function
 * refuses it with "<Name>: float super clips are not supported." */
static int format_ok(const VSVideoInfo *vi, int orFloat) {
    return mvx_vsh_is_constant_video_format(vi) && ((vi->format.bitsPerSample <= 16 && vi->format.sampleType == stInteger) || (orFloat && vi_is_float(vi))) &&
           vi->format.subSamplingW <= 1 && vi->format.subSamplingH <= 1 && (vi->format.colorFamily == cfYUV || vi->format.colorFamily == cfGray);
}
static int super_format_ok(const VSVideoInfo *vi) { return format_ok(vi, 1); }
static int integer_format_ok(const VSVideoInfo *vi) { return format_ok(vi, 0); }

/* ------------------------------------------------------------------------------------------------ device frame cache */

typedef struct DevFrame { int64_t id; void *arena; void *plane[3]; size_t bytes; int pins; uint64_t stamp; uint64_t print;
                         int trusted; /* built by this plugin's own mv.Super (superGetFrame / super_build_device), not uploaded from a host frame that merely carries the id */ } DevFrame;
#define CACHE_MAX 2048
static DevFrame g_cache[CACHE_MAX];
static int g_cache_cap = -1;       /* entries (MVX_VS_CACHE_FRAMES), at most CACHE_MAX */
static size_t g_cache_budget;      /* bytes the cached frames may hold together; 0 = not fixed yet */
static size_t g_cache_bytes;       /* bytes they hold now */
static uint64_t g_stamp = 1;
static int64_t g_next_instance = 1;
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;

/* ONE high-priority non-blocking stream carries every thread's uploads, per-frame kernels (Super, Degrain, ...) and downloads: that
 * work is short and PCIe is serial anyway; the searches run on low-priority streams of their own (one per Analyse instance) and a
 * different priority means a different hardware queue, so a frame's copies never wait behind a 0.3 s search launch.  (A stream per
 * worker thread was measured and is worse: 40 ms to create each, and they share hardware queues with the searches.) */
static void *g_frame_stream;
static int g_frame_stream_tried;
/* MVX_VS_STATS=1: thread-seconds by category, printed with the launch statistics when the plugin is unloaded */
enum { PF_STREAM, PF_UPLOAD, PF_DOWNLOAD, PF_SUPER, PF_SEARCH_WAIT, PF_DEGRAIN, PF_ALLOC, PF_LA_BLOCKED, PF_BUILD_LOCK, PF_GF_SUPER, PF_GF_ANALYSE, PF_GF_DEGRAIN, PF_LA_BUILD, PF_LA_ARENA, PF_LA_LAUNCH, PF_LA_SRCUP, PF_N };
static double g_prof[PF_N];
static long g_prof_n[PF_N];
static int g_prof_on = -1;
static double prof_now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }
static void prof_add(int k, double t0) {
    if (g_prof_on < 0) g_prof_on = getenv("MVX_VS_STATS") != NULL;
    if (!g_prof_on) return;
    const double dt = prof_now() - t0;
    pthread_mutex_lock(&g_lock); g_prof[k] += dt; g_prof_n[k]++; pthread_mutex_unlock(&g_lock);
}
/* MVX_VS_TRACE=1: one line on stderr per look-ahead window event (seconds since the first event) */
static int g_trace_on = -1;
static double g_trace_t0;
static void la_trace(const void *inst, int w, const char *what, double dur) {
    if (g_trace_on < 0) { g_trace_on = getenv("MVX_VS_TRACE") != NULL; g_trace_t0 = prof_now(); }
    if (g_trace_on) fprintf(stderr, "mvtools_vs trace %8.3f  analyse %p window %d %s (%.3f s)\n", prof_now() - g_trace_t0, inst, w, what, dur);
}
/* The per-frame work of a worker thread (its uploads, its Super / Degrain / ... kernels) runs on ONE stream of a small pool
 * (MVX_VS_FRAME_STREAMS, default 4; r3 had ONE for all threads: a thread's kernel then waited behind every other thread's uploads), chosen per
 * thread the first time it asks.  Every getFrame waits for its own stream before it publishes or releases anything, so the streams need no
 * ordering among each other.  640 4K16 frames, lazy super frames: 405 fps with one stream, 481 with four, 508 with eight
 * (profiles/r4_vs_shell_frame_streams.txt); the default mode is bound by its super-frame downloads and does not change. */
#define FRAME_STREAMS_MAX 8
static void *g_frame_streams[FRAME_STREAMS_MAX];
static int g_frame_nstreams, g_frame_next;
static __thread int t_frame_stream = -1;
static void *thread_stream(void) {
    if (!__atomic_load_n(&g_frame_stream_tried, __ATOMIC_ACQUIRE)) {
        pthread_mutex_lock(&g_lock);
        if (!g_frame_stream_tried) {
            const char *e = getenv("MVX_VS_FRAME_STREAMS");
            int n = e ? atoi(e) : 4;
            n = n < 1 ? 1 : n > FRAME_STREAMS_MAX ? FRAME_STREAMS_MAX : n;
            for (int i = 0; i < n; i++) g_frame_streams[i] = mvx_stream_create_priority(1);
            g_frame_stream = g_frame_streams[0];
            g_frame_nstreams = n;
            __atomic_store_n(&g_frame_stream_tried, 1, __ATOMIC_RELEASE);
        }
        pthread_mutex_unlock(&g_lock);
    }
    if (g_frame_nstreams <= 1) return g_frame_stream;
    if (t_frame_stream < 0) t_frame_stream = __atomic_fetch_add(&g_frame_next, 1, __ATOMIC_RELAXED) % g_frame_nstreams;
    return g_frame_streams[t_frame_stream] ? g_frame_streams[t_frame_stream] : g_frame_stream;
}
/* the 131 MB downloads of finished super frames (mv.Super's host frames) run on a stream of their own: they only depend on kernels that
 * were waited for already, and on their own stream they overlap the other threads' uploads (PCIe is full duplex) instead of queueing
 * in front of them */
/* r6: MVX_VS_DL_STREAMS of them (default 2), taken in turn: one stream is one DMA engine's worth of device-to-host bandwidth (~45 GB/s measured), and the 138 MB of super frame
 * per output frame that mv.Super's default mode sends to the host make that engine the bound of the whole graph */
#define DL_STREAMS_MAX 8
static void *g_dl_stream, *g_dl_streams[DL_STREAMS_MAX];
static int g_dl_stream_tried, g_dl_nstreams;
static unsigned g_dl_next;
static void *download_stream(void) {
    if (!__atomic_load_n(&g_dl_stream_tried, __ATOMIC_ACQUIRE)) {
        pthread_mutex_lock(&g_lock);
        if (!g_dl_stream_tried) {
            const char *e = getenv("MVX_VS_DL_STREAMS");
            int want = e ? atoi(e) : 2;
            if (want < 1) want = 1;
            if (want > DL_STREAMS_MAX) want = DL_STREAMS_MAX;
            for (int i = 0; i < want; i++) { void *st = mvx_stream_create_priority(1); if (st) g_dl_streams[g_dl_nstreams++] = st; }
            g_dl_stream = g_dl_nstreams ? g_dl_streams[0] : NULL;
            __atomic_store_n(&g_dl_stream_tried, 1, __ATOMIC_RELEASE);
        }
        pthread_mutex_unlock(&g_lock);
    }
    if (!g_dl_nstreams) return thread_stream();
    return g_dl_streams[__atomic_fetch_add(&g_dl_next, 1u, __ATOMIC_RELAXED) % (unsigned)g_dl_nstreams];
}
/* Error paths: a getFrame that failed after it enqueued work skipped its stream waits, and mvx_dev_free hands a buffer straight to the next
 * caller (no stream ordering in the pool: ADVICE r2) -- so before such a path frees device memory it waits for whatever is still queued on the
 * streams it used.  A no-op when rc == 0. */
static void shell_quiesce(int rc) {
    if (!rc) return;
    (void)mvx_stream_sync(thread_stream());
    for (int i = 0; i < g_dl_nstreams; i++) (void)mvx_stream_sync(g_dl_streams[i]);
}
static int timed_download_on(void *stream, void *dst, ptrdiff_t dp, const void *src, ptrdiff_t sp, size_t rb, size_t rows) {
    const double t0 = prof_now();
    const int rc = mvx_download_2d(dst, dp, src, sp, rb, rows, stream);
    prof_add(PF_DOWNLOAD, t0);
    return rc;
}
static int timed_upload(void *dst, ptrdiff_t dp, const void *src, ptrdiff_t sp, size_t rb, size_t rows) {
    const double t0 = prof_now();
    const int rc = mvx_upload_2d(dst, dp, src, sp, rb, rows, thread_stream());
    prof_add(PF_UPLOAD, t0);
    return rc;
}
static int timed_download(void *dst, ptrdiff_t dp, const void *src, ptrdiff_t sp, size_t rb, size_t rows) {
    const double t0 = prof_now();
    const int rc = mvx_download_2d(dst, dp, src, sp, rb, rows, thread_stream());
    prof_add(PF_DOWNLOAD, t0);
    return rc;
}

/* The device cache is bounded in BYTES: MVX_VS_CACHE_BYTES, else 40 % of what the device has free when the first frame arrives (115 GB
 * of an idle MI355X; less on a smaller or shared GPU) -- and in entries (MVX_VS_CACHE_FRAMES, CACHE_MAX).  The budget limits what is
 * KEPT for later: frames somebody has pinned (a getFrame in progress, the windows of a look-ahead search) are held whatever it says,
 * and unpinned ones are evicted least recently used first to make room.  It should cover the frames a host has in flight (its thread
 * count + twice the temporal radius; with look-ahead two windows per vector clip): a frame that falls out is built or uploaded again.
 * Super clips of different sizes share the budget; when a device allocation fails, unpinned entries are evicted before the shell gives
 * up (shell_alloc). */
static int cache_cap(void) {
    if (g_cache_cap < 0) {
        const char *e = getenv("MVX_VS_CACHE_FRAMES");
        g_cache_cap = e ? atoi(e) : CACHE_MAX;
        if (g_cache_cap > CACHE_MAX) g_cache_cap = CACHE_MAX;
        if (g_cache_cap < 0) g_cache_cap = 0;
    }
    return g_cache_cap;
}
static size_t cache_budget(void) { /* g_lock held */
    if (!g_cache_budget) {
        const char *b = getenv("MVX_VS_CACHE_BYTES");
        double budget = b ? atof(b) : 48.0 * 1024 * 1024 * 1024;
        size_t fr = 0, tot = 0;
        if (!b && mvx_dev_mem_info(&fr, &tot) == 0) budget = 0.4 * (double)fr;
        g_cache_budget = budget < 1.0 ? 1 : (size_t)budget;
        /* evicted arenas must be REUSED, not freed: hipFree synchronises the whole device, i.e. waits for the search launches in flight (0.5 s
         * each) -- a window of 128 new 4K16 super frames evicts 34 GB, more than the pool's default 24 GiB holds, and the frees that followed
         * stalled every request thread for seconds.  The free list may therefore hold a quarter of the device memory. */
        if (tot || mvx_dev_mem_info(&fr, &tot) == 0) mvx_dev_pool_limit(tot / 4);
    }
    return g_cache_budget;
}
/* drops the least recently used unpinned entry; returns its arena (the caller frees it outside the lock) or NULL.  g_lock held. */
static void *cache_evict_lru_locked(void) {
    DevFrame *v = NULL;
    for (int i = 0; i < cache_cap(); i++) {
        DevFrame *e = &g_cache[i];
        if (e->arena && e->pins == 0 && (!v || e->stamp < v->stamp)) v = e;
    }
    if (!v) return NULL;
    void *a = v->arena;
    v->arena = NULL; g_cache_bytes -= v->bytes; v->bytes = 0;
    return a;
}
/* device memory for the shell: on failure the free list of the pool and then unpinned cache entries make room */
static void *shell_alloc(size_t bytes) {
    void *p = mvx_dev_alloc_uninit(bytes);
    while (!p) {
        pthread_mutex_lock(&g_lock);
        void *victim = cache_evict_lru_locked();
        pthread_mutex_unlock(&g_lock);
        if (!victim) break;
        mvx_dev_free(victim);
        mvx_dev_pool_trim(); /* the victim has another size: give it back to the driver */
        p = mvx_dev_alloc_uninit(bytes);
    }
    return p;
}

/* geometry of a super frame on the device: one arena per frame, planes at 256-byte pitches */
/* (every plane is followed by its shadow copies, mvx_super_shadow_frames: the search loads dword-aligned from them) */
typedef struct SuperGeo { const mvx_super *sup; mvx_super_info si; ptrdiff_t pitch[3], shadowStride[3]; size_t off[3]; size_t bytes; int bps, copies; } SuperGeo;

static void super_geo(SuperGeo *g, const mvx_super *s) {
    g->sup = s;
    mvx_super_get_info(s, &g->si);
    g->bps = (g->si.bits + 7) / 8;
    g->copies = 1 + mvx_super_shadow_copies(s);
    for (int p = 0; p < 3; p++) g->pitch[p] = p < g->si.num_planes ? ((ptrdiff_t)g->si.plane_width[p] * g->bps + 255) / 256 * 256 : 0;
    size_t extra[3];
    mvx_super_shadow_bytes(s, g->pitch, extra); /* room behind each plane for its shadow data */
    size_t o = 0;
    for (int p = 0; p < 3; p++) {
        g->off[p] = o; g->shadowStride[p] = 0;
        if (p < g->si.num_planes) {
            g->shadowStride[p] = ((ptrdiff_t)g->pitch[p] * g->si.plane_height[p] + 255) / 256 * 256;
            o += (size_t)g->shadowStride[p] + (extra[p] + 255) / 256 * 256;
        }
    }
    g->bytes = o;
}
/* the shifted copies behind freshly written planes (no-op for 8-bit clips) */
static int super_shadows(const SuperGeo *g, void *const plane[3], void *stream) {
    if (g->copies <= 1) return 0;
    return mvx_super_shadow_frames(g->sup, 1, plane, g->pitch, g->shadowStride, stream);
}
/* cheap fingerprint of a host super frame: a few rows of every plane.  Most filters copy frame props while changing pixels, so the
 * id prop alone does not prove that the cached device copy still matches the frame a consumer was handed. */
static uint64_t frame_print(const VSFrame *f, const SuperGeo *g, const VSAPI *vs) {
    uint64_t h = 1469598103934665603ULL;
    for (int p = 0; p < g->si.num_planes; p++) {
        const int H = g->si.plane_height[p];
        const size_t rb = (size_t)g->si.plane_width[p] * g->bps;
        const int rows[5] = { 0, H / 5, H / 2, (int)((int64_t)H * 4 / 5), H - 1 };
        for (int k = 0; k < 5; k++) {
            const uint8_t *r = vs->getReadPtr(f, p) + (ptrdiff_t)rows[k] * vs->getStride(f, p);
            for (size_t i = 0; i + 8 <= rb; i += 8) { uint64_t v; memcpy(&v, r + i, 8); h = (h ^ v) * 1099511628211ULL; }
        }
    }
    return h;
}

/* returns a pinned cache entry holding frame `id` with that fingerprint, or NULL.  own_bytes != 0: look-up by id alone, for entries this
 * plugin's own mv.Super built (`trusted`) with exactly that layout size -- a frame uploaded from the host under the same id (a filter
 * between mv.Super and its consumer may copy the properties and change the pixels) never answers it. */
static DevFrame *cache_find_ex(int64_t id, uint64_t print, size_t own_bytes) {
    DevFrame *r = NULL;
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < cache_cap(); i++) {
        DevFrame *e = &g_cache[i];
        if (e->arena && e->id == id && (own_bytes ? (e->trusted && e->bytes == own_bytes) : e->print == print)) { r = e; r->pins++; r->stamp = g_stamp++; break; }
    }
    pthread_mutex_unlock(&g_lock);
    return r;
}
static DevFrame *cache_find(int64_t id, uint64_t print) { return cache_find_ex(id, print, 0); }
/* drops the unpinned entries of one mv.Super instance (its free callback) */
static void cache_evict_instance(int64_t instance) {
    void *victims[CACHE_MAX];
    int nv = 0;
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < cache_cap(); i++)
        if (g_cache[i].arena && (g_cache[i].id >> 32) == instance && g_cache[i].pins == 0) { victims[nv++] = g_cache[i].arena; g_cache[i].arena = NULL; g_cache_bytes -= g_cache[i].bytes; g_cache[i].bytes = 0; }
    pthread_mutex_unlock(&g_lock);
    for (int i = 0; i < nv; i++) mvx_dev_free(victims[i]);
}
/* hands a freshly filled arena to the cache (pinned); returns NULL if the cache is full of pinned frames / disabled.  Entries are
 * evicted least recently used first until the new frame fits the byte budget. */
static DevFrame *cache_insert(int64_t id, uint64_t print, void *arena, const SuperGeo *g, int trusted) {
    DevFrame *slot = NULL;
    void *victims[CACHE_MAX];
    int nv = 0;
    pthread_mutex_lock(&g_lock);
    const size_t budget = cache_budget();
    for (int i = 0; i < cache_cap(); i++) { /* a stale unpinned copy of the same frame goes first */
        DevFrame *e = &g_cache[i];
        if (e->arena && e->id == id && e->pins == 0 && (trusted || !e->trusted)) { victims[nv++] = e->arena; e->arena = NULL; g_cache_bytes -= e->bytes; e->bytes = 0; } /* (an upload never displaces the genuine copy) */
    }
    while (g_cache_bytes + g->bytes > budget) {
        void *v = cache_evict_lru_locked();
        if (!v) break;
        victims[nv++] = v;
    }
    /* (still over the budget: everything left is pinned, i.e. needed right now -- the new frame is kept all the same) */
    for (int i = 0; i < cache_cap(); i++) if (!g_cache[i].arena) { slot = &g_cache[i]; break; }
    if (!slot && cache_cap() > 0) { /* every entry in use: recycle the least recently used unpinned one */
        void *v = cache_evict_lru_locked();
        if (v) { victims[nv++] = v; for (int i = 0; i < cache_cap(); i++) if (!g_cache[i].arena) { slot = &g_cache[i]; break; } }
    }
    if (slot) {
        slot->id = id; slot->print = print; slot->arena = arena; slot->bytes = g->bytes; slot->pins = 1; slot->stamp = g_stamp++; slot->trusted = trusted;
        g_cache_bytes += g->bytes;
        for (int p = 0; p < 3; p++) slot->plane[p] = p < g->si.num_planes ? (char *)arena + g->off[p] : NULL;
    }
    pthread_mutex_unlock(&g_lock);
    for (int i = 0; i < nv; i++) mvx_dev_free(victims[i]);
    return slot;
}
static void cache_unpin(DevFrame *e) {
    if (!e) return;
    pthread_mutex_lock(&g_lock);
    e->pins--;
    pthread_mutex_unlock(&g_lock);
}

/* a super frame on the device for the duration of one getFrame: from the cache or uploaded into a temporary arena */
typedef struct DevRef { DevFrame *cached; void *temp; void *plane[3]; } DevRef;

/* MVX_VS_SUPER_LAZY=1 (opt-in, r4): mv.Super hands out frames whose super pixels were never downloaded -- 138 MB per 4K16 frame, three quarters
 * of what the shell moves over PCIe per output frame.  Such a frame carries the SOURCE planes in the top-left corner of its planes (a host copy)
 * and the property MVX_super_lazy; the device copy lives in the cache, and a consumer that does not find it there rebuilds it on the device from
 * the embedded source with the mv.Super instance's own handle.  Only this plugin's filters understand such frames: any other consumer of the
 * super clip would see the source picture in a corner of an otherwise undefined frame -- hence opt-in. */
#define PROP_SUPER_LAZY "MVX_super_lazy"
static int super_lazy(void) { static int v = -1; if (v < 0) { const char *e = getenv("MVX_VS_SUPER_LAZY"); v = e && atoi(e) != 0; } return v; }
static int super_rebuild_lazy(DevRef *r, const VSFrame *f, int64_t id, uint64_t print, const SuperGeo *want, const VSAPI *vs);

static int super_to_device(DevRef *r, const VSFrame *f, const SuperGeo *g, const VSAPI *vs) {
    memset(r, 0, sizeof(*r));
    int err = 0;
    const int64_t id = vs->mapGetInt(vs->getFramePropertiesRO(f), PROP_SUPER_ID, 0, &err);
    const uint64_t print = frame_print(f, g, vs);
    if (!err && (r->cached = cache_find(id, print)) != NULL) {
        for (int p = 0; p < 3; p++) r->plane[p] = r->cached->plane[p];
        return 0;
    }
    {
        int lerr = 0;
        if (!err && vs->mapGetInt(vs->getFramePropertiesRO(f), PROP_SUPER_LAZY, 0, &lerr) == 1 && !lerr) return super_rebuild_lazy(r, f, id, print, g, vs);
    }
    void *arena = shell_alloc(g->bytes);
    if (!arena) return MVX_E_NOMEM;
    void *st = thread_stream();
    int rc = mvx_dev_memset(arena, 0, g->bytes, st); /* zero-filled like the frames mv.Super builds (pitch padding) */
    for (int p = 0; p < g->si.num_planes && !rc; p++) {
        void *d = (char *)arena + g->off[p];
        rc = timed_upload(d, g->pitch[p], vs->getReadPtr(f, p), vs->getStride(f, p), (size_t)g->si.plane_width[p] * g->bps, (size_t)g->si.plane_height[p]);
        r->plane[p] = d;
    }
    if (!rc) rc = super_shadows(g, r->plane, st);
    if (!rc) rc = mvx_stream_sync(st); /* consumers launch on their own streams */
    if (rc) { shell_quiesce(rc); mvx_dev_free(arena); memset(r, 0, sizeof(*r)); return rc; }
    if (!err && (r->cached = cache_insert(id, print, arena, g, 0)) != NULL) return 0; /* keep it for the next consumer (found again by id AND fingerprint only) */
    r->temp = arena;
    return 0;
}
static void dev_release(DevRef *r) {
    if (r->cached) cache_unpin(r->cached);
    if (r->temp) mvx_dev_free(r->temp);
    memset(r, 0, sizeof(*r));
}

/* ------------------------------------------------------------------------------------------------ small helpers */

static int32_t opt_int(const VSMap *in, const char *key, const VSAPI *vs) {
    int err = 0;
    const int v = vs->mapGetIntSaturated(in, key, 0, &err);
    return err ? MVX_UNSET : v;
}
static int64_t opt_int64(const VSMap *in, const char *key, const VSAPI *vs) {
    int err = 0;
    const int64_t v = vs->mapGetInt(in, key, 0, &err);
    return err ? (int64_t)MVX_UNSET : v;
}

/* fields / tff (src/MVAnalyse.c:367-370, MVRecalculate.c:332-335, MVCompensate.c:435,453-454) */
typedef struct FieldOpt { int fields, tff, tffExists; } FieldOpt;

static void field_opt(FieldOpt *o, const VSMap *in, const VSAPI *vs) {
    int e;
    o->fields = !!vs->mapGetInt(in, "fields", 0, &e);
    o->tff = !!vs->mapGetInt(in, "tff", 0, &e);
    o->tffExists = !e;
}

/* parity of frame n: its _Field prop unless tff was passed (src/MVAnalyse.c:135-145); *missing is set when neither exists */
static int frame_top_field(const FieldOpt *o, const VSFrame *f, int n, int *missing, const VSAPI *vs) {
    int e;
    int top = !!vs->mapGetInt(vs->getFramePropertiesRO(f), "_Field", 0, &e);
    if (e && !o->tffExists) *missing = 1;
    if (o->tffExists) top = o->tff ^ (n % 2);
    return top;
}

static int field_shift_of(int srcTop, int refTop, int pel) { /* src/MVAnalyse.c:177 */
    return (srcTop && !refTop) ? pel / 2 : ((refTop && !srcTop) ? -(pel / 2) : 0);
}

/* Super_* props of frame 0 of a super clip -> a geometry-only mvx_super handle (consumers: src/MVAnalyse.c:519-553,
 * src/MVDegrains.cpp:556-581, src/MVCompensate.c:470-500).  `filter` prefixes the reference's messages. */
static mvx_super *super_from_props(VSNode *super, const char *filter, char *error, size_t esz, const VSAPI *vs) {
    char msg[1024];
    const VSFrame *f0 = vs->getFrame(0, super, msg, sizeof(msg));
    if (!f0) { snprintf(error, esz, "%s: failed to retrieve first frame from super clip. Error message: %s", filter, msg); return NULL; }
    const VSMap *props = vs->getFramePropertiesRO(f0);
    int e[6];
    const int height = vs->mapGetIntSaturated(props, "Super_height", 0, &e[0]);
    const int hpad = vs->mapGetIntSaturated(props, "Super_hpad", 0, &e[1]);
    const int vpad = vs->mapGetIntSaturated(props, "Super_vpad", 0, &e[2]);
    const int pel = vs->mapGetIntSaturated(props, "Super_pel", 0, &e[3]);
    const int modeyuv = vs->mapGetIntSaturated(props, "Super_modeyuv", 0, &e[4]);
    const int levels = vs->mapGetIntSaturated(props, "Super_levels", 0, &e[5]);
    vs->freeFrame(f0);
    for (int i = 0; i < 6; i++)
        if (e[i]) {
            snprintf(error, esz, "%s: required properties not found in first frame of super clip. Maybe clip didn't come from mv.Super? Was the first frame trimmed away?", filter);
            return NULL;
        }
    const VSVideoInfo *vi = vs->getVideoInfo(super);
    if (height <= 0 || hpad < 0 || hpad >= vi->width / 2 || vpad < 0 || pel < 1 || pel > 4 || modeyuv < 0 || modeyuv > 7 || levels < 1) {
        snprintf(error, esz, "%s: parameters from super clip appear to be wrong.", filter);
        return NULL;
    }
    mvx_super_args a;
    a.width = vi->width - 2 * hpad; a.height = height; a.bits = vi->format.bitsPerSample;
    a.subsampling_w = vi->format.subSamplingW; a.subsampling_h = vi->format.subSamplingH; a.gray = vi->format.colorFamily == cfGray;
    a.hpad = hpad; a.vpad = vpad; a.pel = pel; a.levels = levels; a.chroma = modeyuv != 1; a.sharp = MVX_UNSET; a.rfilter = MVX_UNSET;
    mvx_super *s = NULL;
    char err[MVX_ERRLEN];
    /* a float super clip (MVX_VS_FLOAT=1) gets the float handle: the filters without a float entry then refuse it with the library's own message */
    if ((vi_is_float(vi) ? mvx_super_create_float : mvx_super_create)(&a, &s, err)) { snprintf(error, esz, "%s: parameters from super clip appear to be wrong.", filter); return NULL; }
    return s;
}

/* src/MVAnalysisData.c:34-64 adataFromVectorClip */
static int adata_from_clip(mvx_analysis_data *ad, VSNode *clip, const char *filter, const char *name, char *error, size_t esz, const VSAPI *vs) {
    char msg[1024];
    const VSFrame *f0 = vs->getFrame(0, clip, msg, sizeof(msg));
    if (!f0) { snprintf(error, esz, "%s: Failed to retrieve first frame from %s. Error message: %s", filter, name, msg); return -1; }
    const VSMap *props = vs->getFramePropertiesRO(f0);
    int err = 0;
    const char *data = vs->mapGetData(props, PROP_ADATA, 0, &err);
    int rc = 0;
    if (err) { snprintf(error, esz, "%s: Property '%s' not found in first frame of %s.", filter, PROP_ADATA, name); rc = -1; }
    else {
        const int size = vs->mapGetDataSize(props, PROP_ADATA, 0, NULL);
        if (size != (int)sizeof(*ad)) { snprintf(error, esz, "%s: Property '%s' in first frame of %s has wrong size (%d instead of %d).", filter, PROP_ADATA, name, size, (int)sizeof(*ad)); rc = -1; }
        else memcpy(ad, data, sizeof(*ad));
    }
    vs->freeFrame(f0);
    return rc;
}
/* src/MVAnalysisData.c:67-99 adataCheckSimilarity */
static int adata_similar(const mvx_analysis_data *a, const mvx_analysis_data *b, const char *filter, const char *n1, const char *n2, char *error, size_t esz) {
    const char *what = NULL;
    if (a->nWidth != b->nWidth) what = "widths";
    if (a->nHeight != b->nHeight) what = "heights";
    if (a->nBlkSizeX != b->nBlkSizeX || a->nBlkSizeY != b->nBlkSizeY) what = "block sizes";
    if (a->nPel != b->nPel) what = "pel precision";
    if (a->nOverlapX != b->nOverlapX || a->nOverlapY != b->nOverlapY) what = "overlap";
    if (a->xRatioUV != b->xRatioUV) what = "horizontal subsampling";
    if (a->yRatioUV != b->yRatioUV) what = "vertical subsampling";
    if (a->bitsPerSample != b->bitsPerSample) what = "bit depths";
    if (!what) return 0;
    snprintf(error, esz, "%s: %s and %s have different %s.", filter, n1, n2, what);
    return -1;
}

/* MVTools_vectors of a vector-clip frame -> device.  The array states its own size in its first int (gopGetArraySize,
 * GroupOfPlanes.c:167-174); clips made with divide carry an extra array the level formula does not describe.  blob_check is the validation alone (the fields of a
 * multi vector clip go through it too). */
static int blob_check(const char *blob, int n, const mvx_analysis_data *ad) {
    int stated = 0;
    if (n >= 8) memcpy(&stated, blob, sizeof(stated));
    if (n < 8 || stated != n) return MVX_E_ARG;
    /* the planes' own size headers must tile the array exactly (fgopUpdate walks them, Fakery.c:112-123): a spliced or truncated
     * property must not send the device readers out of bounds */
    int planes = 0, lastOff = 0;
    for (int off = 8; off < n; planes++) {
        int psz = 0;
        if (off + 4 > n) return MVX_E_ARG;
        memcpy(&psz, blob + off, sizeof(psz));
        if (psz < 4 + 16 || (psz - 4) % 16 || psz > n - off) return MVX_E_ARG;
        lastOff = off;
        off += psz;
    }
    if (ad) { /* the readers skip nLvCount - 1 planes and then read nBlkX * nBlkY vectors */
        int off = 8;
        for (int i = ad->nLvCount - 1; i >= 1 && off < n; i--) { int psz; memcpy(&psz, blob + off, sizeof(psz)); off += psz; }
        if (planes < ad->nLvCount || off > lastOff || n - off < 4 + ad->nBlkX * ad->nBlkY * 16) return MVX_E_ARG;
    }
    return 0;
}
static int blob_to_device(void **dblob, int *size, const mvx_analysis_data *ad, const VSFrame *vf, const VSAPI *vs) {
    int e = 0;
    const VSMap *props = vs->getFramePropertiesRO(vf);
    const char *blob = vs->mapGetData(props, PROP_VECTORS, 0, &e);
    *dblob = NULL;
    if (e) return MVX_E_ARG;
    const int n = vs->mapGetDataSize(props, PROP_VECTORS, 0, NULL);
    if (blob_check(blob, n, ad)) return MVX_E_ARG;
    *dblob = shell_alloc((size_t)n);
    if (!*dblob) return MVX_E_NOMEM;
    if (timed_upload(*dblob, n, blob, n, (size_t)n, 1)) return MVX_E_DEVICE; /* complete on return: the prop memory goes away with the frame */
    if (size) *size = n;
    return 0;
}

/* the planes of a host frame -> one device arena.  Returns 0 or an MVX_E_* code; the copies are complete on return (the host frame
 * may be released right away) */
static int upload_plane_set(void *dst[3], void **arena, const VSFrame *f, const ptrdiff_t pitch[3], int nplanes, int bps, const VSAPI *vs) {
    size_t off[3], total = 0;
    for (int p = 0; p < nplanes; p++) { off[p] = total; total += (size_t)pitch[p] * vs->getFrameHeight(f, p); }
    *arena = shell_alloc(total);
    for (int p = 0; p < 3; p++) dst[p] = NULL;
    if (!*arena) return MVX_E_NOMEM;
    int rc = 0;
    for (int p = 0; p < nplanes && !rc; p++) {
        dst[p] = (char *)*arena + off[p];
        rc = timed_upload(dst[p], pitch[p], vs->getReadPtr(f, p), vs->getStride(f, p), (size_t)vs->getFrameWidth(f, p) * bps, (size_t)vs->getFrameHeight(f, p));
    }
    return rc;
}

/* ------------------------------------------------------------------------------------------------ mv.Super */

typedef struct SuperData { VSNode *node, *pelclip; VSVideoInfo vi; mvx_super *sup; SuperGeo geo; ptrdiff_t srcPitch[3], pelPitch[3]; int32_t pelMode; int64_t instance; } SuperData;

/* The output nodes of this plugin's own mv.Super filters.  A consumer whose `super` argument IS one of them (pointer identity: no
 * filter in between that could have changed pixels while copying the props) may build the super frames it needs on the device itself
 * from the 5x smaller SOURCE frames -- what mv.Analyse's look-ahead does -- and trust cached device frames by their id alone. */
#define SUPER_REG_MAX 64
static struct { VSNode *out; struct SuperData *d; } g_supers[SUPER_REG_MAX];
static void super_register(VSNode *out, SuperData *d) {
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < SUPER_REG_MAX; i++) if (!g_supers[i].out) { g_supers[i].out = out; g_supers[i].d = d; break; }
    pthread_mutex_unlock(&g_lock);
}
static void super_unregister(SuperData *d) {
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < SUPER_REG_MAX; i++) if (g_supers[i].d == d) { g_supers[i].out = NULL; g_supers[i].d = NULL; }
    pthread_mutex_unlock(&g_lock);
}
static SuperData *super_lookup(VSNode *out) {
    SuperData *d = NULL;
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < SUPER_REG_MAX; i++) if (g_supers[i].out == out) d = g_supers[i].d;
    pthread_mutex_unlock(&g_lock);
    return d;
}
static SuperData *super_by_instance(int64_t instance) {
    SuperData *d = NULL;
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < SUPER_REG_MAX; i++) if (g_supers[i].d && g_supers[i].d->instance == instance) d = g_supers[i].d;
    pthread_mutex_unlock(&g_lock);
    return d;
}
/* lazy super frames (MVX_VS_SUPER_LAZY): the source picture in the top-left corner of every plane; the rows the fingerprint samples are defined */
static void lazy_fill(VSFrame *dst, const VSFrame *src, const SuperGeo *g, const VSAPI *vs) {
    for (int p = 0; p < g->si.num_planes; p++) {
        const int H = g->si.plane_height[p];
        const size_t rb = (size_t)g->si.plane_width[p] * g->bps;
        const int rows[5] = { 0, H / 5, H / 2, (int)((int64_t)H * 4 / 5), H - 1 }; /* (= frame_print's) */
        uint8_t *dp = vs->getWritePtr(dst, p);
        const ptrdiff_t ds = vs->getStride(dst, p), ss = vs->getStride(src, p);
        /* the whole plane is defined (zero outside the embedded source): newVideoFrame hands out uninitialised heap, and a consumer that is
         * not this plugin must neither see stale memory nor a frame that differs from run to run */
        for (int y = 0; y < H; y++) memset(dp + (ptrdiff_t)y * ds, 0, rb);
        (void)rows;
        const uint8_t *sp = vs->getReadPtr(src, p);
        const size_t wb = (size_t)vs->getFrameWidth(src, p) * g->bps;
        const int h = vs->getFrameHeight(src, p);
        for (int y = 0; y < h; y++) memcpy(dp + (ptrdiff_t)y * ds, sp + (ptrdiff_t)y * ss, wb);
    }
    vs->mapSetInt(vs->getFramePropertiesRW(dst), PROP_SUPER_LAZY, 1, maReplace);
}
/* a consumer found no device copy of a lazy frame: rebuild it from the embedded source with the handle of the mv.Super instance that made it */
static int super_rebuild_lazy(DevRef *r, const VSFrame *f, int64_t id, uint64_t print, const SuperGeo *want, const VSAPI *vs) {
    SuperData *sd = super_by_instance(id >> 32);
    if (!sd || sd->pelMode) return MVX_E_ARG; /* (its mv.Super instance is gone: cannot happen while a consumer holds the node) */
    const SuperGeo *g = &sd->geo;
    /* the id comes from frame properties: a stale or foreign one may name a live instance with ANOTHER layout -- the planes built below must be the
     * ones the consumer's kernels will address */
    if (g->bytes != want->bytes || g->copies != want->copies || g->bps != want->bps || g->si.num_planes != want->si.num_planes) return MVX_E_ARG;
    for (int p = 0; p < g->si.num_planes; p++)
        if (g->pitch[p] != want->pitch[p] || g->off[p] != want->off[p] || g->shadowStride[p] != want->shadowStride[p] ||
            g->si.plane_width[p] != want->si.plane_width[p] || g->si.plane_height[p] != want->si.plane_height[p]) return MVX_E_ARG;
    size_t off[3], total = 0;
    int w[3], h[3];
    for (int p = 0; p < g->si.num_planes; p++) {
        w[p] = p ? g->si.width / g->si.xRatioUV : g->si.width; h[p] = p ? g->si.height / g->si.yRatioUV : g->si.height;
        off[p] = total; total += (size_t)sd->srcPitch[p] * (size_t)h[p];
    }
    void *srcArena = shell_alloc(total), *arena = shell_alloc(g->bytes), *dsrc[3] = { NULL, NULL, NULL };
    int rc = (!srcArena || !arena) ? MVX_E_NOMEM : 0;
    void *st = thread_stream();
    if (!rc) rc = mvx_dev_memset(arena, 0, g->bytes, st);
    for (int p = 0; p < g->si.num_planes && !rc; p++) {
        dsrc[p] = (char *)srcArena + off[p];
        rc = timed_upload(dsrc[p], sd->srcPitch[p], vs->getReadPtr(f, p), vs->getStride(f, p), (size_t)w[p] * g->bps, (size_t)h[p]);
        r->plane[p] = (char *)arena + g->off[p];
    }
    if (!rc) {
        if (g->copies > 1) rc = mvx_super_frames_shadow(sd->sup, 1, (const void *const *)dsrc, sd->srcPitch, (void *const *)r->plane, g->pitch, g->shadowStride, st);
        else rc = mvx_super_frames(sd->sup, 1, (const void *const *)dsrc, sd->srcPitch, (void *const *)r->plane, g->pitch, st);
    }
    if (!rc) rc = mvx_stream_sync(st); else (void)mvx_stream_sync(st);
    if (srcArena) mvx_dev_free(srcArena);
    if (rc) { shell_quiesce(rc); if (arena) mvx_dev_free(arena); memset(r, 0, sizeof(*r)); return rc; }
    if ((r->cached = cache_insert(id, print, arena, g, 0)) != NULL) return 0;
    r->temp = arena;
    return 0;
}
/* builds the device super frames of `n` SOURCE frames in one batch (uploads, then one mvx_super_frames_shadow call) and hands them
 * to the cache, pinned; frames that are cached already are only pinned.  out[i] = the pinned entry of frame nums[i].  One builder at a
 * time: six vector clips ask for the same frames.  Returns 0 or an MVX_E_* code (entries pinned so far are released on failure). */
static pthread_mutex_t g_build_mu = PTHREAD_MUTEX_INITIALIZER;
#define BUILD_THREADS 8
static long env_long_early(const char *name, long def) { const char *e = getenv(name); return e ? atol(e) : def; }
typedef struct BuildJob { SuperData *sd; const VSAPI *vs; const int *miss; int nmiss; const VSFrame *const *srcs; void **srcArena, **arena; const void **sp; void **dp; int next, rc; pthread_mutex_t mu; void *st; } BuildJob;
static void *build_worker(void *arg) { /* uploads source frames and prepares their (zero-filled) super arenas, one frame at a time */
    BuildJob *j = (BuildJob *)arg;
    const SuperGeo *g = &j->sd->geo;
    void *st = j->st; /* the BUILDER's stream: the arenas' memsets must be ordered before the super kernels it launches there (a helper thread's own stream of the pool is not) */
    for (;;) {
        pthread_mutex_lock(&j->mu);
        const int k = (j->rc || j->next >= j->nmiss) ? -1 : j->next++;
        pthread_mutex_unlock(&j->mu);
        if (k < 0) return NULL;
        const int i = j->miss[k];
        void *d3[3];
        double tq = prof_now();
        int rc = upload_plane_set(d3, &j->srcArena[k], j->srcs[i], j->sd->srcPitch, g->si.num_planes, g->bps, j->vs);
        prof_add(PF_LA_SRCUP, tq);
        for (int p = 0; p < 3; p++) j->sp[k * 3 + p] = d3[p];
        tq = prof_now();
        if (!rc && !(j->arena[k] = shell_alloc(g->bytes))) rc = MVX_E_NOMEM;
        prof_add(PF_LA_ARENA, tq);
        if (!rc) rc = mvx_dev_memset(j->arena[k], 0, g->bytes, st);
        for (int p = 0; p < g->si.num_planes && !rc; p++) j->dp[k * 3 + p] = (char *)j->arena[k] + g->off[p];
        if (rc) { pthread_mutex_lock(&j->mu); if (!j->rc) j->rc = rc; pthread_mutex_unlock(&j->mu); }
    }
}
static int super_build_device(SuperData *sd, int n, const int *nums, const VSFrame *const *srcs, DevFrame **out, const VSAPI *vs) {
    const SuperGeo *g = &sd->geo;
    int rc = 0, nmiss = 0;
    const double tl = prof_now();
    pthread_mutex_lock(&g_build_mu);
    prof_add(PF_BUILD_LOCK, tl);
    int *miss = (int *)malloc(sizeof(int) * (size_t)n);
    void **srcArena = (void **)calloc((size_t)n, sizeof(void *)), **arena = (void **)calloc((size_t)n, sizeof(void *));
    const void **sp = (const void **)calloc((size_t)n * 3, sizeof(void *));
    void **dp = (void **)calloc((size_t)n * 3, sizeof(void *));
    if (!miss || !srcArena || !arena || !sp || !dp) rc = MVX_E_NOMEM;
    for (int i = 0; i < n; i++) out[i] = NULL;
    for (int i = 0; i < n && !rc; i++) {
        out[i] = cache_find_ex((sd->instance << 32) | (uint32_t)nums[i], 0, g->bytes);
        if (!out[i]) miss[nmiss++] = i;
    }
    void *st = thread_stream();
    const double tp = prof_now();
    if (!rc && nmiss) { /* the uploads (a host memcpy into pinned staging + a DMA each) are spread over a few helper threads: a window of 64 4K16
                         * frames is 1.6 GB, which one thread moves in ~0.4 s -- as long as it takes to consume the window */
        BuildJob job = { sd, vs, miss, nmiss, srcs, srcArena, arena, sp, dp, 0, 0, PTHREAD_MUTEX_INITIALIZER, st };
        pthread_t th[BUILD_THREADS];
        int want = (int)env_long_early("MVX_VS_BUILD_THREADS", 4);
        if (want < 1) want = 1;
        if (want > BUILD_THREADS) want = BUILD_THREADS;
        int nth = nmiss >= 2 * want ? want : (nmiss > 1 ? 2 : 1), started = 0;
        if (nth > want) nth = want;
        for (int t = 1; t < nth; t++) if (pthread_create(&th[started], NULL, build_worker, &job) == 0) started++;
        build_worker(&job);
        for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
        rc = job.rc;
    }
    if (!rc && nmiss) {
        if (g->copies > 1) rc = mvx_super_frames_shadow(sd->sup, nmiss, sp, sd->srcPitch, dp, g->pitch, g->shadowStride, st);
        else rc = mvx_super_frames(sd->sup, nmiss, sp, sd->srcPitch, dp, g->pitch, st);
    }
    if (!rc && nmiss) rc = mvx_stream_sync(st);
    else if (rc && nmiss) (void)mvx_stream_sync(st); /* (part of the work may be queued: the arenas below go back to a pool that knows nothing of streams) */
    prof_add(PF_SUPER, tp);
    for (int k = 0; k < nmiss; k++) {
        if (srcArena && srcArena[k]) mvx_dev_free(srcArena[k]);
        if (!rc) {
            const int i = miss[k];
            out[i] = cache_insert((sd->instance << 32) | (uint32_t)nums[i], 0, arena[k], g, 1); /* (print 0: superGetFrame fills it in when it hands the host frame out) */
            if (!out[i]) { rc = MVX_E_NOMEM; mvx_dev_free(arena[k]); }
        } else if (arena && arena[k]) mvx_dev_free(arena[k]);
    }
    if (rc) for (int i = 0; i < n; i++) if (out[i]) { cache_unpin(out[i]); out[i] = NULL; }
    free(miss); free(srcArena); free(arena); free(sp); free(dp);
    pthread_mutex_unlock(&g_build_mu);
    return rc;
}

static void super_frame_props(VSFrame *dst, int n, int64_t id, const SuperGeo *g, const VSAPI *vs) {
    VSMap *props = vs->getFramePropertiesRW(dst);
    if (n == 0) { /* src/MVSuper.c:111-120 */
        vs->mapSetInt(props, "Super_height", g->si.height, maReplace);
        vs->mapSetInt(props, "Super_hpad", g->si.hpad, maReplace);
        vs->mapSetInt(props, "Super_vpad", g->si.vpad, maReplace);
        vs->mapSetInt(props, "Super_pel", g->si.pel, maReplace);
        vs->mapSetInt(props, "Super_modeyuv", g->si.modeYUV, maReplace);
        vs->mapSetInt(props, "Super_levels", g->si.levels, maReplace);
    }
    vs->mapSetInt(props, PROP_SUPER_ID, id, maReplace); /* (harmless extra prop; frames without it are uploaded by the consumers) */
}

static const VSFrame *VS_CC superGetFrame(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    SuperData *d = (SuperData *)inst;
    if (reason == arInitial) { /* src/MVSuper.c:47-52 */
        vs->requestFrameFilter(n, d->node, ctx);
        if (d->pelMode) vs->requestFrameFilter(n, d->pelclip, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const double tgf = prof_now();
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    const SuperGeo *g = &d->geo;
    const int64_t id = (d->instance << 32) | (uint32_t)n;
    DevFrame *have = d->pelMode ? NULL : cache_find_ex(id, 0, g->bytes); /* built on the device already (a vector clip's look-ahead): only the download is left */
    if (have) {
        int rc2 = 0;
        VSFrame *dst2 = vs->newVideoFrame(&d->vi.format, d->vi.width, d->vi.height, src, core);
        if (super_lazy()) lazy_fill(dst2, src, g, vs); /* (the pixels stay on the device) */
        else for (int p = 0; p < g->si.num_planes && !rc2; p++)
            rc2 = timed_download_on(download_stream(), vs->getWritePtr(dst2, p), vs->getStride(dst2, p), have->plane[p], g->pitch[p], (size_t)g->si.plane_width[p] * g->bps, (size_t)g->si.plane_height[p]);
        vs->freeFrame(src);
        if (rc2) { cache_unpin(have); vs->freeFrame(dst2); vs->setFilterError(mvx_last_error(), ctx); return NULL; }
        super_frame_props(dst2, n, id, g, vs);
        const uint64_t pr = frame_print(dst2, g, vs);
        pthread_mutex_lock(&g_lock); have->print = pr; pthread_mutex_unlock(&g_lock);
        cache_unpin(have);
        prof_add(PF_GF_SUPER, tgf);
        return dst2;
    }
    void *srcArena = NULL, *pelArena = NULL, *dsrc[3], *dpel[3] = { NULL, NULL, NULL }, *ddst[3] = { NULL, NULL, NULL };
    int rc = upload_plane_set(dsrc, &srcArena, src, d->srcPitch, g->si.num_planes, g->bps, vs);
    const VSFrame *pf = d->pelMode ? vs->getFrameFilter(n, d->pelclip, ctx) : NULL; /* src/MVSuper.c:62-64 */
    if (pf && !rc) rc = upload_plane_set(dpel, &pelArena, pf, d->pelPitch, g->si.num_planes, g->bps, vs);
    void *st = thread_stream();
    double tp = prof_now();
    void *arena = rc ? NULL : shell_alloc(g->bytes);
    prof_add(PF_ALLOC, tp);
    tp = prof_now();
    if (!rc && !arena) rc = MVX_E_NOMEM;
    if (!rc) rc = mvx_dev_memset(arena, 0, g->bytes, st); /* zero-filled: only the defined rectangles are written (MVSuper.c:73 memsets too) */
    if (!rc) {
        for (int p = 0; p < g->si.num_planes; p++) ddst[p] = (char *)arena + g->off[p];
        if (!d->pelMode && g->copies > 1) /* the level-0 kernels write their share of the shadow planes themselves */
            rc = mvx_super_frames_shadow(d->sup, 1, (const void *const *)dsrc, d->srcPitch, (void *const *)ddst, g->pitch, g->shadowStride, st);
        else if (mvx_super_is_float(d->sup)) /* (one level, no shadow copies, never a pelclip: superCreate) */
            rc = mvx_super_frames(d->sup, 1, (const void *const *)dsrc, d->srcPitch, (void *const *)ddst, g->pitch, st);
        else {
            rc = mvx_super_frames_pelclip(d->sup, 1, (const void *const *)dsrc, d->srcPitch, (const void *const *)dpel, d->pelPitch, d->pelMode, (void *const *)ddst, g->pitch, st);
            if (!rc) rc = super_shadows(g, ddst, st);
        }
    }
    if (!rc) rc = mvx_stream_sync(st);
    prof_add(PF_SUPER, tp);
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi.format, d->vi.width, d->vi.height, src, core);
        if (super_lazy() && !d->pelMode) lazy_fill(dst, src, g, vs);
        else {
            for (int p = 0; p < g->si.num_planes && !rc; p++)
                rc = timed_download_on(download_stream(), vs->getWritePtr(dst, p), vs->getStride(dst, p), ddst[p], g->pitch[p], (size_t)g->si.plane_width[p] * g->bps, (size_t)g->si.plane_height[p]);
        }
    }
    shell_quiesce(rc);
    if (srcArena) mvx_dev_free(srcArena);
    if (pelArena) mvx_dev_free(pelArena);
    if (pf) vs->freeFrame(pf);
    vs->freeFrame(src);
    if (rc) {
        if (arena) mvx_dev_free(arena);
        if (dst) vs->freeFrame(dst);
        vs->setFilterError(mvx_last_error(), ctx);
        return NULL;
    }
    super_frame_props(dst, n, id, g, vs);
    /* the device copy stays resident for the consumers */
    DevFrame *e = cache_insert(id, frame_print(dst, g, vs), arena, g, 1);
    if (e) cache_unpin(e); else mvx_dev_free(arena);
    prof_add(PF_GF_SUPER, tgf);
    return dst;
}

static void VS_CC superFree(void *inst, VSCore *core, const VSAPI *vs) {
    (void)core;
    SuperData *d = (SuperData *)inst;
    vs->freeNode(d->node);
    if (d->pelclip) vs->freeNode(d->pelclip);
    super_unregister(d);
    cache_evict_instance(d->instance); /* its device-resident frames are of no use to anybody now */
    mvx_super_destroy(d->sup);
    free(d);
}

/* ------------------------------------------------------------------------------------------------ start-up on a background thread (r6)
 * The HIP runtime (0.25-0.3 s), this library's code objects (~0.1 s at the first launch) and the page-locked staging buffers (~20 ms each) come up on a thread started when the
 * plugin is loaded, while the host is still reading its script / opening its clips.  Two rules keep that safe: (1) every filter-creation function first waits until the RUNTIME
 * is up (what a synchronous start would have cost it anyway) -- so a host that exits after a creation error never tears the process down under a thread that is inside the
 * runtime's initialisation (the runtime's own exit handlers run before any handler registered earlier: measured, a segmentation fault at exit with the error message still in the
 * stdio buffer); (2) as soon as the runtime is up, and BEFORE it lets the waiting creation functions go on, the thread registers an exit handler -- which therefore runs before the
 * runtime's -- that waits for the rest of the warm-up.  What the rules do not cover is a host that calls exit() without having called a creation function and without freeing its
 * core (freeing it unloads the plugin, whose destructor joins the thread): such a host sets MVX_VS_WARMUP=0, as the mini host does for `list` and `error` (minihost.c, leave).
 * MVX_VS_WARMUP=0 turns the thread off, MVX_VS_WARM_STAGES = staging buffers to page-lock (default 48 = 768 MiB: what a 4K session allocates within its first second). */
static pthread_t g_warm_thread;
static int g_warm_started, g_warm_runtime_up, g_warm_done; /* (atomics: __atomic_*) */
static void warm_join(void) {
    if (__atomic_exchange_n(&g_warm_started, 0, __ATOMIC_ACQ_REL)) pthread_join(g_warm_thread, NULL);
}
static void *warmup_thread(void *arg) {
    (void)arg;
    (void)mvx_warmup(-1);         /* the runtime (no device: the filters report that when they are used) */
    atexit(warm_join);            /* (registered after the runtime's own handlers, so it runs before them; and before a creation function may go on and exit) */
    __atomic_store_n(&g_warm_runtime_up, 1, __ATOMIC_RELEASE);
    const char *e = getenv("MVX_VS_WARM_STAGES");
    (void)mvx_warmup(e ? atoi(e) : 48); /* code objects, staging buffers */
    __atomic_store_n(&g_warm_done, 1, __ATOMIC_RELEASE);
    return NULL;
}
static void warm_barrier(void) { /* at the top of every *Create: the runtime is up (or no warm-up runs) */
    while (__atomic_load_n(&g_warm_started, __ATOMIC_ACQUIRE) && !__atomic_load_n(&g_warm_runtime_up, __ATOMIC_ACQUIRE)) { struct timespec t = { 0, 2000000 }; nanosleep(&t, NULL); }
}
__attribute__((destructor)) static void warm_unload(void) { warm_join(); } /* (dlclose without exit) */

static void VS_CC superCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    VSNode *node = vs->mapGetNode(in, "clip", 0, 0);
    const VSVideoInfo *vi = vs->getVideoInfo(node);
    /* a float clip (MVX_VS_FLOAT=1) of a constant Gray or YUV format goes to mvx_super_create_float whatever its subsampling: levels, pel, sharp, rfilter, the format and
     * the padding are then refused by the library, in the library's order */
    const int isFloat = vi_is_float(vi) && mvx_vsh_is_constant_video_format(vi) && (vi->format.colorFamily == cfYUV || vi->format.colorFamily == cfGray);
    if (!isFloat && (!mvx_vsh_is_constant_video_format(vi) || vi->format.bitsPerSample > 16 || vi->format.sampleType != stInteger || vi->format.subSamplingW > 1 ||
        vi->format.subSamplingH > 1 || (vi->format.colorFamily != cfYUV && vi->format.colorFamily != cfGray))) {
        /* argument-value errors come first in the reference (MVSuper.c:177-192): let the library report them on a dummy format */
        mvx_super_args t = { 64, 64, 8, 1, 1, 0, opt_int(in, "hpad", vs), opt_int(in, "vpad", vs), opt_int(in, "pel", vs), opt_int(in, "levels", vs), opt_int(in, "chroma", vs), opt_int(in, "sharp", vs), opt_int(in, "rfilter", vs) };
        mvx_super *ts = NULL; char terr[MVX_ERRLEN];
        if (mvx_super_create(&t, &ts, terr)) vs->mapSetError(out, terr);
        else { mvx_super_destroy(ts); vs->mapSetError(out, "Super: input clip must be GRAY, 420, 422, 440, or 444, up to 16 bits, with constant dimensions."); }
        vs->freeNode(node);
        return;
    }
    mvx_super_args a = { vi->width, vi->height, vi->format.bitsPerSample, vi->format.subSamplingW, vi->format.subSamplingH, vi->format.colorFamily == cfGray,
                         opt_int(in, "hpad", vs), opt_int(in, "vpad", vs), opt_int(in, "pel", vs), opt_int(in, "levels", vs), opt_int(in, "chroma", vs),
                         opt_int(in, "sharp", vs), opt_int(in, "rfilter", vs) };
    if (a.chroma != MVX_UNSET) a.chroma = !!a.chroma;
    mvx_super *sup = NULL;
    char err[MVX_ERRLEN];
    if ((isFloat ? mvx_super_create_float : mvx_super_create)(&a, &sup, err)) { vs->mapSetError(out, err); vs->freeNode(node); return; }
    /* src/MVSuper.c:229-256 */
    int perr = 0;
    int32_t pelMode = 0;
    VSNode *pelclip = vs->mapGetNode(in, "pelclip", 0, &perr);
    if (perr) pelclip = NULL;
    if (pelclip && isFloat) { /* (the library's pelclip entry refuses a float super clip: one message here, where the pelclip's own checks sit) */
        vs->mapSetError(out, "Super: pelclip is not supported on float clips.");
        mvx_super_destroy(sup); vs->freeNode(node); vs->freeNode(pelclip);
        return;
    }
    if (pelclip) {
        const VSVideoInfo *pvi = vs->getVideoInfo(pelclip);
        const int same = pvi->format.colorFamily == vi->format.colorFamily && pvi->format.sampleType == vi->format.sampleType &&
                         pvi->format.bitsPerSample == vi->format.bitsPerSample && pvi->format.subSamplingW == vi->format.subSamplingW &&
                         pvi->format.subSamplingH == vi->format.subSamplingH;
        err[0] = 0;
        if (!mvx_vsh_is_constant_video_format(pvi) || !same) snprintf(err, sizeof(err), "Super: pelclip must have the same format as the input clip, and it must have constant dimensions.");
        else mvx_super_pelclip_mode(sup, pvi->width, pvi->height, &pelMode, err);
        if (err[0]) { vs->mapSetError(out, err); mvx_super_destroy(sup); vs->freeNode(node); vs->freeNode(pelclip); return; }
    }
    SuperData *d = (SuperData *)calloc(1, sizeof(*d));
    d->node = node; d->sup = sup; d->vi = *vi;
    d->pelclip = pelclip; d->pelMode = pelMode;
    super_geo(&d->geo, sup);
    d->vi.width = d->geo.si.super_width; d->vi.height = d->geo.si.super_height;
    const int bps = d->geo.bps;
    for (int p = 0; p < 3; p++) {
        const int w = p ? vi->width >> vi->format.subSamplingW : vi->width;
        d->srcPitch[p] = ((ptrdiff_t)w * bps + 255) / 256 * 256;
        if (pelMode) {
            const VSVideoInfo *pvi = vs->getVideoInfo(pelclip);
            const int pw = p ? pvi->width >> vi->format.subSamplingW : pvi->width;
            d->pelPitch[p] = ((ptrdiff_t)pw * bps + 255) / 256 * 256;
        }
    }
    pthread_mutex_lock(&g_lock);
    d->instance = g_next_instance++;
    pthread_mutex_unlock(&g_lock);
    VSFilterDependency deps[2] = { { node, rpStrictSpatial }, { pelclip, rpStrictSpatial } };
    vs->createVideoFilter(out, "Super", &d->vi, superGetFrame, superFree, fmParallel, deps, pelMode ? 2 : 1, d, core);
    { /* remember the node the core made for this instance (identity only: no reference is kept) */
        int e = 0;
        VSNode *o = vs->mapGetNode(out, "clip", 0, &e);
        if (o && !e) { super_register(o, d); vs->freeNode(o); }
    }
}

/* ------------------------------------------------------------------------------------------------ mv.Analyse */

/* Combining queue: the getFrame calls of concurrent worker threads become ONE mvx_analyse_frames launch.  The first thread to
 * arrive leads: it waits for others -- until `maxBatch` requests are queued, or no new request has arrived for a quiet period, or a
 * total budget is used up -- takes the whole queue, launches it on the instance's stream, waits for it and wakes the others up.
 * Requests arriving meanwhile form the next batch.  Quiet period and budget follow the duration of the previous launch (1/8 and
 * 1/2 of it, at least MVX_VS_BATCH_WAIT_US, the quiet period at most MVX_VS_BATCH_QUIET_MAX_US): a 4K search takes ~0.3 s whether it
 * carries one chain or five hundred, so the frames a host delivers a few milliseconds apart are worth waiting for. */
typedef struct AnReq { mvx_analyse_job job; int rc, done; struct AnReq *next; } AnReq;
typedef struct Combiner {
    pthread_mutex_t mu; pthread_cond_t done, more;
    AnReq *head, *tail; int n, leader;
    int maxBatch; long waitUs, quietMaxUs; /* a few streams: the next batch may start while the previous one runs */
    long lastUs; /* duration of the previous launch: a search of few chains takes as long as one of hundreds, so waiting a fraction of it for more requests is cheap */
    long batches, jobs, largest; /* statistics (MVX_VS_STATS=1 prints them when the filter is freed) */
} Combiner;

/* Look-ahead (mv.Analyse whose `super` argument is this plugin's own mv.Super node).  A search is a serial chain per frame that
 * takes ~0.45 s at 4K however few chains a launch carries, so a vector clip is computed a WINDOW of B consecutive
 * frames at a time: the first request that touches window w also asks for the SOURCE frames (25 MB each at 4K16, not the 131 MB
 * super frames) of w and of the next two windows, builds their super frames on the device only, and launches one search per window on
 * the instance's low-priority streams; the windows ahead are gathered, built and searched while the frames of w are being consumed.  Every other request of the window just waits
 * for the launch that is already running (GPU work only: nothing it waits for needs a host worker thread) and copies its blob out
 * of the window's host array.  The request protocol stays the reference's (MVAnalyse.c:84-113: everything a frame needs is asked
 * for at arInitial and fetched at arAllFramesReady); the extra requests go to the source clip, declared as a second dependency. */
#define LA_SLOTS 6
enum { LW_EMPTY, LW_BUILDING, LW_LAUNCHED, LW_SYNCING, LW_READY, LW_FAILED };
typedef struct LaWindow { int w, state, first, count, users, rc; void *dblobs; size_t dstride; DevFrame **pins; int npins; void *stream; } LaWindow; /* dblobs: the window's vectors, on the device until the slot is recycled */
/* The engine has two users, mv.Analyse and mv.AnalyseN.  What differs between them is below the line: how many frames a window needs before and after its own (the
 * arithmetic is mvx_vs_window.h's), how many bytes of vectors a frame has, and the launch itself.  A launch callback gets the window's inputs on the device -- pins[i] is
 * source frame lo + i, the last of the nn entries the fixed frame where there is one outside [lo, hi], top[i] its parity -- and `count` frames' room at dblobs; it enqueues
 * ONE library call on `stream` and does not wait for it. */
typedef struct LaLaunch { int first, count, lo, hi, nn; const int *top; DevFrame *const *pins; void *dblobs; void *stream; } LaLaunch;
typedef struct LookAhead { int on, B, depth; volatile int started; /* a window of this instance has been launched (r6: the request that starts the FIRST one starts no window ahead) */ volatile int degraded; /* a window ran out of device memory: new requests take the per-frame path */ VSNode *srcNode; SuperData *sd; pthread_mutex_t mu; pthread_cond_t cv; LaWindow win[LA_SLOTS];
    /* ---- the user's */
    void *owner; int numFrames, before, after, fixed; /* fixed: a static reference frame every window needs (mv.Analyse with delta <= 0), else -1 */
    size_t frameBytes; const FieldOpt *fo; int (*enqueue)(void *owner, const LaLaunch *l); } LookAhead;
#define LA_DEPTH_MAX 3
typedef struct LaReq { int w, hold[1 + LA_DEPTH_MAX], want[1 + LA_DEPTH_MAX]; } LaReq; /* the frame data of a request that goes through the windows (one that does not has none) */

typedef struct AnalyseData { VSNode *node; const VSVideoInfo *vi; mvx_super *sup; SuperGeo geo; mvx_analyse *an; mvx_analysis_data ad; int blobSize; FieldOpt fo; Combiner cb; LookAhead la; } AnalyseData;

static long env_long(const char *name, long def) { const char *e = getenv(name); return e ? atol(e) : def; }

/* totals over all instances, printed when the plugin is unloaded (MVX_VS_STATS=1): a host need not free its nodes before it exits */
static long g_stat_launches, g_stat_jobs, g_stat_largest, g_stat_instances;
/* ... and of mv.AnalyseN's windows: a line of their own, only when a window was launched */
static long g_statn_windows, g_statn_frames, g_statn_chains, g_statn_largest;
__attribute__((destructor)) static void print_stats(void) {
    if (env_long("MVX_VS_STATS", 0) && g_stat_instances)
    {
        fprintf(stderr, "mvtools_vs: Analyse instances=%ld launches=%ld jobs=%ld largest_batch=%ld\n", g_stat_instances, g_stat_launches, g_stat_jobs, g_stat_largest);
        static const char *nm[PF_N] = { "stream_create", "upload", "download", "super_kernels", "search_wait", "degrain", "dev_alloc", "lookahead_blocked", "build_lock",
                                        "getframe_super", "getframe_analyse", "getframe_degrain", "window_build", "window_arena_alloc", "window_launch_call", "window_source_upload" };
        fprintf(stderr, "mvtools_vs: thread-seconds");
        for (int k = 0; k < PF_N; k++) fprintf(stderr, " %s=%.2f/%ld", nm[k], g_prof[k], g_prof_n[k]);
        fprintf(stderr, "\n");
    }
    if (env_long("MVX_VS_STATS", 0) && g_statn_windows)
        fprintf(stderr, "mvtools_vs: AnalyseN windows=%ld frames=%ld chains=%ld largest_window=%ld\n", g_statn_windows, g_statn_frames, g_statn_chains, g_statn_largest);
}

/* Streams of the search launches, shared by every mv.Analyse instance and handed out round robin.  The runtime maps streams onto a few
 * hardware queues per priority level, in creation order, and launches that share a queue run one after the other: with four streams per
 * instance the six instances of a Degrain3 graph put the six searches of a window on the SAME queue (traced: 128-chain launches enqueued
 * together finished 0.6 s apart, two at a time).  One pool makes consecutive launches land on different queues; the HOST should run with
 * GPU_MAX_HW_QUEUES >= SEARCH_STREAMS (the mini host sets 16 unless the user chose a value).  Priority: MVX_VS_SEARCH_PRIO (-1 lowest = default, 0, 1);
 * a NULL entry (the default stream) still works, it only serialises. */
#define SEARCH_STREAMS 12
static void *g_search_stream[SEARCH_STREAMS];
static unsigned g_search_next;
static int g_search_made;
static void *search_stream_next(void) {
    pthread_mutex_lock(&g_lock);
    if (!g_search_made) {
        g_search_made = 1;
        for (int i = 0; i < SEARCH_STREAMS; i++) g_search_stream[i] = mvx_stream_create_priority((int)env_long("MVX_VS_SEARCH_PRIO", -1));
    }
    void *st = g_search_stream[g_search_next++ % SEARCH_STREAMS];
    pthread_mutex_unlock(&g_lock);
    return st;
}
static void combiner_init(Combiner *c) {
    memset(c, 0, sizeof(*c));
    pthread_mutex_init(&c->mu, NULL); pthread_cond_init(&c->done, NULL); pthread_cond_init(&c->more, NULL);
    /* priority of the search streams: MVX_VS_SEARCH_PRIO (-1 lowest = default, 0, 1); NULL (the default stream) still works, it only serialises the launches */
    pthread_mutex_lock(&g_lock); g_stat_instances++; pthread_mutex_unlock(&g_lock);
    c->maxBatch = (int)env_long("MVX_VS_BATCH_MAX", 1024);
    c->waitUs = env_long("MVX_VS_BATCH_WAIT_US", 2000);
    c->quietMaxUs = env_long("MVX_VS_BATCH_QUIET_MAX_US", 30000);
    if (c->maxBatch < 1) c->maxBatch = 1;
}
static void combiner_free(Combiner *c, const char *what) {
    (void)what;
    pthread_mutex_destroy(&c->mu); pthread_cond_destroy(&c->done); pthread_cond_destroy(&c->more);
}
/* blocks until the request's blob is computed; returns its MVX_* code */
static int combiner_submit(Combiner *c, mvx_analyse *an, AnReq *r) {
    pthread_mutex_lock(&c->mu);
    r->next = NULL; r->done = 0;
    if (c->tail) c->tail->next = r; else c->head = r;
    c->tail = r; c->n++;
    if (c->leader) { /* follower */
        pthread_cond_signal(&c->more); /* the leader restarts its quiet period */
        while (!r->done) pthread_cond_wait(&c->done, &c->mu);
        pthread_mutex_unlock(&c->mu);
        return r->rc;
    }
    c->leader = 1;
    if (c->waitUs > 0 && c->n < c->maxBatch) {
        long quiet = c->lastUs / 8, budget = c->lastUs / 2;
        if (quiet > c->quietMaxUs) quiet = c->quietMaxUs;
        if (quiet < c->waitUs) quiet = c->waitUs;
        if (budget < c->waitUs) budget = c->waitUs;
        struct timespec t0, now, ts;
        clock_gettime(CLOCK_REALTIME, &t0);
        while (c->n < c->maxBatch) {
            clock_gettime(CLOCK_REALTIME, &now);
            const long used = (now.tv_sec - t0.tv_sec) * 1000000L + (now.tv_nsec - t0.tv_nsec) / 1000;
            if (used >= budget) break;
            const long w = quiet < budget - used ? quiet : budget - used;
            ts = now;
            ts.tv_nsec += (w % 1000000) * 1000; ts.tv_sec += w / 1000000 + ts.tv_nsec / 1000000000; ts.tv_nsec %= 1000000000;
            const int n0 = c->n;
            if (pthread_cond_timedwait(&c->more, &c->mu, &ts) == ETIMEDOUT && c->n == n0) break; /* quiet: nobody else is about to arrive */
        }
    }
    AnReq *list = c->head;
    const int n = c->n;
    c->head = c->tail = NULL; c->n = 0; c->leader = 0; /* the next arrival leads the next batch while this one runs */
    void *stream = search_stream_next();
    c->batches++; c->jobs += n; if (n > c->largest) c->largest = n;
    pthread_mutex_unlock(&c->mu);
    pthread_mutex_lock(&g_lock);
    g_stat_launches++; g_stat_jobs += n; if (n > g_stat_largest) g_stat_largest = n;
    pthread_mutex_unlock(&g_lock);
    int rc = 0;
    mvx_analyse_job *jobs = (mvx_analyse_job *)malloc(sizeof(mvx_analyse_job) * (size_t)n);
    if (!jobs) rc = MVX_E_NOMEM;
    else {
        int i = 0;
        for (AnReq *q = list; q; q = q->next) jobs[i++] = q->job;
        struct timespec a, b;
        clock_gettime(CLOCK_MONOTONIC, &a);
        rc = mvx_analyse_frames(an, n, jobs, stream);
        if (!rc) rc = mvx_stream_sync(stream);
        clock_gettime(CLOCK_MONOTONIC, &b);
        free(jobs);
        pthread_mutex_lock(&c->mu);
        c->lastUs = (b.tv_sec - a.tv_sec) * 1000000L + (b.tv_nsec - a.tv_nsec) / 1000;
        pthread_mutex_unlock(&c->mu);
    }
    pthread_mutex_lock(&c->mu);
    for (AnReq *q = list; q;) { AnReq *nx = q->next; q->rc = rc; q->done = 1; q = nx; } /* (q may be freed by its owner once done) */
    pthread_cond_broadcast(&c->done);
    pthread_mutex_unlock(&c->mu);
    return rc;
}

static int analyse_nref(const AnalyseData *d, int n) { /* src/MVAnalyse.c:84-104 */
    if (d->ad.nDeltaFrame > 0) return n + (d->ad.isBackward ? d->ad.nDeltaFrame : -d->ad.nDeltaFrame);
    return -d->ad.nDeltaFrame;
}

/* ---- look-ahead helpers (d->la.mu held where noted) */
static void la_window_release(LaWindow *s) { /* frees what a finished / failed window holds; the slot becomes EMPTY */
    for (int i = 0; i < s->npins; i++) cache_unpin(s->pins[i]);
    free(s->pins); s->pins = NULL; s->npins = 0;
    if (s->dblobs) { mvx_dev_free(s->dblobs); s->dblobs = NULL; }
    s->state = LW_EMPTY; s->count = 0; s->rc = 0;
}
/* the slot of window w, recycled from an older finished window if nobody uses it; NULL if it is taken.  mu held. */
static LaWindow *la_slot(LookAhead *la, int w) {
    LaWindow *s = &la->win[mvx_win_slot(w, LA_SLOTS)];
    if (s->w == w) return s;
    if (s->users || s->state == LW_BUILDING || s->state == LW_LAUNCHED || s->state == LW_SYNCING) return NULL;
    la_window_release(s);
    s->w = w;
    return s;
}
/* source frames window v needs: [*lo, *hi] and, for a static reference, the frame *fixed (else -1) */
static void la_inputs(const LookAhead *la, int v, int *lo, int *hi, int *fixed) {
    int first, count;
    mvx_win_inputs(v, la->B, la->numFrames, la->before, la->after, &first, &count, lo, hi);
    *fixed = la->fixed;
}
static void la_request_inputs(const LookAhead *la, int v, VSFrameContext *ctx, const VSAPI *vs) {
    int lo, hi, fixed;
    la_inputs(la, v, &lo, &hi, &fixed);
    for (int k = lo; k <= hi; k++) vs->requestFrameFilter(k, la->srcNode, ctx);
    if (fixed >= 0 && (fixed < lo || fixed > hi)) vs->requestFrameFilter(fixed, la->srcNode, ctx);
}
/* builds the super frames of window v on the device and enqueues its search (does not wait for it) */
static int la_launch(LookAhead *la, LaWindow *s, int v, VSFrameContext *ctx, const VSAPI *vs) {
    int first, count, lo, hi;
    mvx_win_inputs(v, la->B, la->numFrames, la->before, la->after, &first, &count, &lo, &hi);
    const int fixed = la->fixed;
    const double tl0 = prof_now();
    const int extra = fixed >= 0 && (fixed < lo || fixed > hi);
    const int nn = hi - lo + 1 + extra;
    int *nums = (int *)malloc(sizeof(int) * (size_t)nn), *top = (int *)calloc((size_t)nn, sizeof(int));
    const VSFrame **srcs = (const VSFrame **)calloc((size_t)nn, sizeof(VSFrame *));
    DevFrame **pins = (DevFrame **)calloc((size_t)nn, sizeof(DevFrame *));
    int rc = (!nums || !top || !srcs || !pins) ? MVX_E_NOMEM : 0, missing = 0;
    for (int i = 0; i < nn && !rc; i++) {
        nums[i] = i < hi - lo + 1 ? lo + i : fixed;
        srcs[i] = vs->getFrameFilter(nums[i], la->srcNode, ctx);
        if (!srcs[i]) { rc = MVX_E_ARG; break; }
        top[i] = frame_top_field(la->fo, srcs[i], nums[i], &missing, vs); /* mv.Super copies the props of its source frame (MVSuper.c:104) */
    }
    if (!rc && missing && la->fo->fields) rc = -1000; /* reported by the caller with the reference's message */
    la_trace(la->owner, v, "source frames fetched", prof_now() - tl0);
    { const double tq = prof_now(); if (!rc) rc = super_build_device(la->sd, nn, nums, srcs, pins, vs); prof_add(PF_LA_BUILD, tq); la_trace(la->owner, v, "super frames on the device", prof_now() - tq); }
    for (int i = 0; i < nn; i++) if (srcs && srcs[i]) vs->freeFrame(srcs[i]);
    void *dblobs = rc ? NULL : shell_alloc(la->frameBytes * (size_t)count);
    /* the window's vectors stay on the device; every request downloads its own 2.7 MB when it is served.  (Bringing a whole window to the
     * host at once was tried both ways: a synchronous 350 MB download by the first waiter stalled all request threads six times per window,
     * and page-locked per-slot arrays for an asynchronous copy cost 0.4 s of hipHostMalloc each, during which every HIP call of the process
     * waits.) */
    if (!rc && !dblobs) rc = MVX_E_NOMEM;
    if (!rc) {
        s->stream = search_stream_next();
        const LaLaunch l = { first, count, lo, hi, nn, top, pins, dblobs, s->stream };
        const double tq = prof_now();
        rc = la->enqueue(la->owner, &l);
        prof_add(PF_LA_LAUNCH, tq);
        la_trace(la->owner, v, "search enqueued", prof_now() - tl0);
    }
    if (rc) {
        shell_quiesce(rc);
        if (s->stream) (void)mvx_stream_sync(s->stream);
        for (int i = 0; i < nn; i++) if (pins && pins[i]) cache_unpin(pins[i]);
        free(pins);
        if (dblobs) mvx_dev_free(dblobs);
    } else { s->pins = pins; s->npins = nn; s->dblobs = dblobs; s->dstride = la->frameBytes; s->first = first; s->count = count; }
    free(nums); free(top); free(srcs);
    return rc;
}
/* waits until window s is READY (or FAILED): the first waiter synchronises the window's stream */
static int la_wait(LookAhead *la, LaWindow *s) {
    pthread_mutex_lock(&la->mu);
    for (;;) {
        if (s->state == LW_READY || s->state == LW_FAILED || s->state == LW_EMPTY) break;
        if (s->state == LW_LAUNCHED) {
            s->state = LW_SYNCING;
            pthread_mutex_unlock(&la->mu);
            const double t0 = prof_now();
            const int rc = mvx_stream_sync(s->stream);
            prof_add(PF_SEARCH_WAIT, t0);
            la_trace(la->owner, s->w, "first waiter saw the search finish", prof_now() - t0);
            pthread_mutex_lock(&la->mu);
            for (int i = 0; i < s->npins; i++) cache_unpin(s->pins[i]);
            free(s->pins); s->pins = NULL; s->npins = 0;
            s->rc = rc; s->state = rc ? LW_FAILED : LW_READY;
            pthread_cond_broadcast(&la->cv);
            continue;
        }
        { const double tb = prof_now(); pthread_cond_wait(&la->cv, &la->mu); prof_add(PF_LA_BLOCKED, tb); } /* BUILDING / SYNCING: somebody is on it */
    }
    const int rc = s->state == LW_READY ? 0 : (s->rc ? s->rc : MVX_E_DEVICE);
    pthread_mutex_unlock(&la->mu);
    return rc;
}
static void la_release_req(LookAhead *la, LaReq *r) {
    if (!r) return;
    pthread_mutex_lock(&la->mu);
    for (int i = 0; i <= LA_DEPTH_MAX; i++) if (r->hold[i]) la->win[mvx_win_slot(r->w + i, LA_SLOTS)].users--;
    pthread_mutex_unlock(&la->mu);
    free(r);
}
/* arInitial of the request for frame n of a clip with windows: its frame data, and what it asks for -- frame n of `self` (the vector clip's frame is a copy of the super
 * frame, MVAnalyse.c:224) and the source frames of the windows it will start.  0: no slot / no memory, this request takes the per-frame path and *fd stays NULL */
static int la_request(LookAhead *la, int n, VSNode *self, void **fd, VSFrameContext *ctx, const VSAPI *vs) {
    LaReq *r = (LaReq *)calloc(1, sizeof(LaReq));
    if (!r) return 0;
    r->w = mvx_win_of(n, la->B);
    pthread_mutex_lock(&la->mu);
    LaWindow *s0 = la->degraded ? NULL : la_slot(la, r->w);
    if (s0) {
        s0->users++; r->hold[0] = 1; r->want[0] = s0->state == LW_EMPTY;
        /* (r6: not the request that starts an instance's FIRST window -- mv.DegrainN's creation reads frame 0 of every vector clip, and the windows ahead of
         * the first instances' frame 0 kept the GPU from the later instances' first windows: 0.8 s of graph construction for six clips; the windows ahead are
         * started by the next request, a moment later) */
        for (int i = 1; la->started && i <= la->depth && (r->w + i) * la->B < la->numFrames; i++) { /* the windows ahead: whoever sees them empty first starts them */
            LaWindow *s1 = la_slot(la, r->w + i);
            if (s1 && s1->state == LW_EMPTY) { s1->users++; r->hold[i] = 1; r->want[i] = 1; }
        }
    }
    pthread_mutex_unlock(&la->mu);
    if (!s0) { free(r); return 0; }
    *fd = r;
    vs->requestFrameFilter(n, self, ctx);
    /* one source frame of the window that will be started next: by the time some request sees that window empty and asks
     * for all of its frames, the requests of this window have had the host produce them, in parallel */
    { const int ahead = n + (la->depth + 1) * la->B; if (ahead < la->numFrames) vs->requestFrameFilter(ahead, la->srcNode, ctx); }
    for (int i = 0; i <= LA_DEPTH_MAX; i++) if (r->want[i]) { la_trace(la->owner, r->w + i, "source frames requested", 0.0); la_request_inputs(la, r->w + i, ctx, vs); }
    return 1;
}
/* arAllFramesReady of such a request: starts the windows whose frames it asked for and waits for its own, *win (READY when this returns 0) */
static int la_serve(LookAhead *la, const LaReq *r, LaWindow **win, VSFrameContext *ctx, const VSAPI *vs) {
    int rc = 0;
    for (int i = 0; i <= LA_DEPTH_MAX && !rc; i++) {
        if (!r->want[i]) continue;
        LaWindow *s = &la->win[mvx_win_slot(r->w + i, LA_SLOTS)];
        int mine = 0;
        pthread_mutex_lock(&la->mu);
        if (s->state == LW_EMPTY) { s->state = LW_BUILDING; mine = 1; }
        pthread_mutex_unlock(&la->mu);
        if (!mine) continue;
        const int lrc = la_launch(la, s, r->w + i, ctx, vs);
        pthread_mutex_lock(&la->mu);
        s->rc = lrc; s->state = lrc ? LW_FAILED : LW_LAUNCHED;
        la->started = 1;
        if (lrc == MVX_E_NOMEM) la->degraded = 1; /* (the requests already waiting for this window fail -- their reference frames were never asked for -- but nothing after them does) */
        pthread_cond_broadcast(&la->cv);
        pthread_mutex_unlock(&la->mu);
        if (lrc && i == 0) rc = lrc;
    }
    *win = &la->win[mvx_win_slot(r->w, LA_SLOTS)];
    if (!rc) rc = la_wait(la, *win);
    return rc;
}
/* what creation decides: on with windows of B frames and `depth` of them ahead, unless what they hold would not fit the device (MVX_VS_LOOKAHEAD_AUTOSIZE=0: not asked).
 * superBytes / blobBytes / slots: see mvx_win_bytes; half of the free memory is left to the other vector clips' share, the consumers' frames and the allocator's pool */
static void la_size(LookAhead *la, long B, double superBytes, double blobBytes, int slots) {
    la->on = 1; la->B = (int)(B > 512 ? 512 : B);
    /* windows started ahead of the one being consumed.  Two: gathering a window's source frames and building its super frames
     * takes a host about as long as consuming a window does, and the search itself another ~0.5 s */
    la->depth = (int)env_long("MVX_VS_LOOKAHEAD_DEPTH", 2);
    if (la->depth < 0) la->depth = 0;
    if (la->depth > LA_DEPTH_MAX) la->depth = LA_DEPTH_MAX;
    size_t fr = 0, tot = 0;
    if (env_long("MVX_VS_LOOKAHEAD_AUTOSIZE", 1) && mvx_dev_mem_info(&fr, &tot) == 0 && fr)
        la->on = mvx_win_fit(&la->B, &la->depth, la->before + la->after > 0 ? la->before + la->after : 1, superBytes, blobBytes, slots, 0.5 * (double)fr); /* (0: not even one small window: the per-frame path) */
}
static void la_open(LookAhead *la, VSNode *srcNode, const VSAPI *vs) {
    la->srcNode = vs->addNodeRef(srcNode);
    pthread_mutex_init(&la->mu, NULL); pthread_cond_init(&la->cv, NULL);
    for (int i = 0; i < LA_SLOTS; i++) la->win[i].w = -1;
}
/* the windows' pins go before the nodes: freeing the super node may run mv.Super's free callback, which drops its unpinned frames from the cache */
static void la_drain(LookAhead *la) {
    for (int i = 0; i < LA_SLOTS; i++) {
        LaWindow *s = &la->win[i];
        if (s->state == LW_LAUNCHED) (void)mvx_stream_sync(s->stream); /* nobody came for it */
        la_window_release(s);
    }
}
static void la_close(LookAhead *la, const VSAPI *vs) {
    vs->freeNode(la->srcNode);
    pthread_mutex_destroy(&la->mu); pthread_cond_destroy(&la->cv);
}

/* r6: the vectors of a look-ahead window stay on the device until its slot is recycled; a consumer of this plugin (mv.DegrainN) that finds the window of frame n still there
 * reads them where they are instead of uploading the 2.7 MB property the vector frame carries (six of them per 4K Degrain3 frame).  The vector FRAME is unchanged -- any
 * other consumer reads its properties as before -- and when the window is gone the consumer falls back on them too.  The registry maps the node the core made for an
 * mv.Analyse instance to the instance (identity only, like g_supers; a consumer holds a reference to the node for as long as it may ask). */
#define ANALYSE_REG_MAX 256
static struct { VSNode *out; AnalyseData *d; } g_analyses[ANALYSE_REG_MAX];
static void analyse_register(VSNode *out, AnalyseData *d) {
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < ANALYSE_REG_MAX; i++) if (!g_analyses[i].out) { g_analyses[i].out = out; g_analyses[i].d = d; break; }
    pthread_mutex_unlock(&g_lock);
}
static void analyse_unregister(AnalyseData *d) {
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < ANALYSE_REG_MAX; i++) if (g_analyses[i].d == d) { g_analyses[i].out = NULL; g_analyses[i].d = NULL; }
    pthread_mutex_unlock(&g_lock);
}
static AnalyseData *analyse_lookup(VSNode *out) {
    AnalyseData *d = NULL;
    pthread_mutex_lock(&g_lock);
    for (int i = 0; i < ANALYSE_REG_MAX; i++) if (g_analyses[i].out == out) d = g_analyses[i].d;
    pthread_mutex_unlock(&g_lock);
    return d;
}
/* the device copy of frame n's vectors, its window pinned (la_device_blob_release), or NULL */
static const void *la_device_blob(LookAhead *la, int n, LaWindow **held) {
    *held = NULL;
    if (!la || !la->on) return NULL;
    const void *p = NULL;
    pthread_mutex_lock(&la->mu);
    LaWindow *s = &la->win[mvx_win_slot(mvx_win_of(n, la->B), LA_SLOTS)];
    if (s->w == mvx_win_of(n, la->B) && s->state == LW_READY && s->dblobs && n >= s->first && n < s->first + s->count) {
        s->users++; *held = s;
        p = (const char *)s->dblobs + s->dstride * (size_t)(n - s->first);
    }
    pthread_mutex_unlock(&la->mu);
    return p;
}
static void la_device_blob_release(LookAhead *la, LaWindow *held) {
    if (!held) return;
    pthread_mutex_lock(&la->mu);
    held->users--;
    pthread_mutex_unlock(&la->mu);
}
/* mv.Analyse's launch: one job per frame of the window */
static int analyse_enqueue(void *owner, const LaLaunch *l) {
    AnalyseData *d = (AnalyseData *)owner;
    mvx_analyse_job *jobs = (mvx_analyse_job *)calloc((size_t)l->count, sizeof(mvx_analyse_job));
    if (!jobs) return MVX_E_NOMEM;
    for (int i = 0; i < l->count; i++) {
        const int k = l->first + i, nref = analyse_nref(d, k);
        const int haveRef = nref >= 0 && nref < d->vi->numFrames;
        const int is = k - l->lo, ir = !haveRef ? -1 : (nref >= l->lo && nref <= l->hi) ? nref - l->lo : l->nn - 1;
        for (int p = 0; p < 3; p++) { jobs[i].src[p] = l->pins[is]->plane[p]; jobs[i].ref[p] = haveRef ? l->pins[ir]->plane[p] : NULL; }
        jobs[i].blob = (char *)l->dblobs + d->la.frameBytes * (size_t)i;
        jobs[i].field_shift = (haveRef && d->fo.fields && d->ad.nPel > 1 && (d->ad.nDeltaFrame % 2)) ? field_shift_of(l->top[is], l->top[ir], d->ad.nPel) : 0;
    }
    const int rc = mvx_analyse_frames(d->an, l->count, jobs, l->stream);
    free(jobs);
    pthread_mutex_lock(&g_lock);
    g_stat_launches++; g_stat_jobs += l->count; if (l->count > g_stat_largest) g_stat_largest = l->count;
    pthread_mutex_unlock(&g_lock);
    return rc;
}

static const VSFrame *VS_CC analyseGetFrame(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    AnalyseData *d = (AnalyseData *)inst;
    const int nref = analyse_nref(d, n);
    const int haveRef = nref >= 0 && nref < d->vi->numFrames;
    if (d->la.on) {
        if (reason == arInitial) {
            if (la_request(&d->la, n, d->node, fd, ctx, vs)) return NULL;
            /* (no slot / no memory: this request takes the per-frame path below) */
        } else if (*fd) {
            LaReq *r = (LaReq *)*fd;
            *fd = NULL;
            if (reason != arAllFramesReady) { la_release_req(&d->la, r); return NULL; } /* arError */
            const double tgf = prof_now();
            LaWindow *s = NULL;
            int rc = la_serve(&d->la, r, &s, ctx, vs);
            const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
            VSFrame *dst = NULL;
            char *blob = rc ? NULL : (char *)malloc((size_t)d->blobSize);
            if (!rc && !blob) rc = MVX_E_NOMEM;
            /* (r4: the window's search was waited for; on the download stream the copy does not queue behind other threads' uploads -- PCIe is full duplex) */
            if (!rc) rc = timed_download_on(download_stream(), blob, d->blobSize, (const char *)s->dblobs + s->dstride * (size_t)(n - s->first), d->blobSize, (size_t)d->blobSize, 1);
            if (!rc && src) { /* src/MVAnalyse.c:224-239 */
                dst = vs->copyFrame(src, core);
                VSMap *props = vs->getFramePropertiesRW(dst);
                vs->mapSetData(props, PROP_ADATA, (const char *)&d->ad, sizeof(d->ad), dtBinary, maReplace);
                vs->mapSetData(props, PROP_VECTORS, blob, d->blobSize, dtBinary, maReplace);
            } else
                vs->setFilterError(rc == -1000 ? "Analyse: _Field property not found in input frame. Therefore, you must pass tff argument." :
                                   rc == MVX_E_NOMEM ? "Analyse: out of memory." : mvx_last_error(), ctx);
            free(blob);
            if (src) vs->freeFrame(src);
            la_release_req(&d->la, r);
            prof_add(PF_GF_ANALYSE, tgf);
            return dst;
        }
    }
    if (reason == arInitial) {
        if (haveRef && nref < n) vs->requestFrameFilter(nref, d->node, ctx);
        vs->requestFrameFilter(n, d->node, ctx);
        if (haveRef && nref >= n && nref != n) vs->requestFrameFilter(nref, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    const VSFrame *ref = haveRef ? vs->getFrameFilter(nref, d->node, ctx) : NULL;
    int fieldShift = 0;
    { /* src/MVAnalyse.c:135-179 */
        int missing = 0;
        const int srcTop = frame_top_field(&d->fo, src, n, &missing, vs);
        const int refTop = ref ? frame_top_field(&d->fo, ref, nref, &missing, vs) : 0;
        if (missing && d->fo.fields) {
            vs->setFilterError("Analyse: _Field property not found in input frame. Therefore, you must pass tff argument.", ctx);
            if (ref) vs->freeFrame(ref);
            vs->freeFrame(src);
            return NULL;
        }
        if (ref && d->fo.fields && d->ad.nPel > 1 && (d->ad.nDeltaFrame % 2)) fieldShift = field_shift_of(srcTop, refTop, d->ad.nPel);
    }
    DevRef ds, dr;
    memset(&dr, 0, sizeof(dr));
    int rc = super_to_device(&ds, src, &d->geo, vs);
    if (!rc && ref) rc = super_to_device(&dr, ref, &d->geo, vs);
    void *dblob = rc ? NULL : shell_alloc((size_t)d->blobSize);
    char *blob = (char *)malloc((size_t)d->blobSize);
    if (!rc && (!dblob || !blob)) rc = MVX_E_NOMEM;
    if (!rc) {
        AnReq req;
        memset(&req, 0, sizeof(req));
        for (int p = 0; p < 3; p++) { req.job.src[p] = ds.plane[p]; req.job.ref[p] = ref ? dr.plane[p] : NULL; }
        req.job.blob = dblob;
        req.job.field_shift = fieldShift;
        const double t0 = prof_now();
        rc = combiner_submit(&d->cb, d->an, &req); /* one launch for all the frames requested right now */
        prof_add(PF_SEARCH_WAIT, t0);
        if (!rc) rc = timed_download(blob, d->blobSize, dblob, d->blobSize, (size_t)d->blobSize, 1);
        if (!rc) rc = mvx_stream_sync(thread_stream());
    }
    shell_quiesce(rc);
    dev_release(&ds); dev_release(&dr);
    if (dblob) mvx_dev_free(dblob);
    if (ref) vs->freeFrame(ref);
    VSFrame *dst = NULL;
    if (!rc) { /* src/MVAnalyse.c:224-239 */
        dst = vs->copyFrame(src, core);
        VSMap *props = vs->getFramePropertiesRW(dst);
        vs->mapSetData(props, PROP_ADATA, (const char *)&d->ad, sizeof(d->ad), dtBinary, maReplace);
        vs->mapSetData(props, PROP_VECTORS, blob, d->blobSize, dtBinary, maReplace);
    } else
        vs->setFilterError(rc == MVX_E_NOMEM ? "Analyse: out of memory." : mvx_last_error(), ctx);
    free(blob);
    vs->freeFrame(src);
    return dst;
}

static void VS_CC analyseFree(void *inst, VSCore *core, const VSAPI *vs) {
    (void)core;
    AnalyseData *d = (AnalyseData *)inst;
    analyse_unregister(d);
    if (d->la.on) la_drain(&d->la);
    vs->freeNode(d->node);
    if (d->la.on) la_close(&d->la, vs);
    combiner_free(&d->cb, "Analyse");
    mvx_analyse_destroy(d->an);
    mvx_super_destroy(d->sup);
    free(d);
}

static void VS_CC analyseCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    static const char *keys[] = { "blksize", "blksizev", "levels", "search", "searchparam", "pelsearch", "isb", "lambda", "chroma", "delta", "truemotion",
                                  "lsad", "plevel", "global", "pnew", "pzero", "pglobal", "overlap", "overlapv", "divide", "badsad", "badrange", "opt",
                                  "meander", "trymany", "fields", "tff", "search_coarse", "dct" };
    mvx_analyse_args a;
    int32_t *av = (int32_t *)&a;
    for (size_t i = 0; i < sizeof(keys) / sizeof(keys[0]); i++) av[i] = opt_int(in, keys[i], vs);
    VSNode *node = vs->mapGetNode(in, "super", 0, 0);
    const VSVideoInfo *vi = vs->getVideoInfo(node);
    char err[1200];
    if (!super_format_ok(vi)) {
        vs->mapSetError(out, "Analyse: super clip must be GRAY, 420, 422, 440, or 444, up to 16 bits, with constant dimensions.");
        vs->freeNode(node);
        return;
    }
    mvx_super *sup = super_from_props(node, "Analyse", err, sizeof(err), vs);
    if (!sup) { vs->mapSetError(out, err); vs->freeNode(node); return; }
    AnalyseData *d = (AnalyseData *)calloc(1, sizeof(*d));
    d->node = node; d->vi = vi; d->sup = sup;
    field_opt(&d->fo, in, vs);
    super_geo(&d->geo, sup);
    char lerr[MVX_ERRLEN];
    if (mvx_analyse_create(&a, sup, vi->numFrames, d->geo.pitch, &d->an, lerr)) {
        vs->mapSetError(out, lerr);
        mvx_super_destroy(sup); vs->freeNode(node); free(d);
        return;
    }
    mvx_analyse_get_data(d->an, &d->ad);
    d->blobSize = mvx_analyse_blob_size(d->an);
    if (d->geo.copies > 1) mvx_analyse_set_ref_shadow(d->an, d->geo.shadowStride); /* every device super frame of this shell carries its copies */
    combiner_init(&d->cb);
    /* before the first launch has been timed: a chain walks every block of every level, a few microseconds each */
    d->cb.lastUs = (long)((double)d->ad.nBlkX * d->ad.nBlkY * 4.0 / 3.0 * 2.5);
    VSFilterDependency deps[2] = { { node, rpGeneral }, { NULL, rpGeneral } };
    int ndeps = 1;
    { /* look-ahead when `super` is this plugin's own mv.Super node (MVX_VS_LOOKAHEAD = window length in frames, 0 = off; default 128) */
        SuperData *sd = super_lookup(node);
        const long B = env_long("MVX_VS_LOOKAHEAD", 128);
        if (sd && !sd->pelMode && B > 0 && vi->numFrames > 1 && cache_cap() > 0) { /* (no device cache, no windows: they live in it) */
            const int delta = d->ad.nDeltaFrame;
            d->la.sd = sd; d->la.owner = d; d->la.numFrames = vi->numFrames; d->la.fo = &d->fo; d->la.enqueue = analyse_enqueue;
            d->la.before = delta > 0 && !d->ad.isBackward ? delta : 0; d->la.after = delta > 0 && d->ad.isBackward ? delta : 0;
            d->la.fixed = delta <= 0 && -delta < vi->numFrames ? -delta : -1;
            d->la.frameBytes = ((size_t)d->blobSize + 255) / 256 * 256;
            /* what the windows in flight pin must fit the device: every window holds B + delta super frames (with their shadow planes) and B blobs */
            la_size(&d->la, B, (double)sd->geo.bytes * 1.2 + (double)d->blobSize, 0.0, 0);
        }
        if (d->la.on) {
            la_open(&d->la, sd->node, vs);
            deps[1].source = d->la.srcNode; ndeps = 2;
        }
    }
    vs->createVideoFilter(out, "Analyse", vi, analyseGetFrame, analyseFree, fmParallel, deps, ndeps, d, core);
    if (d->la.on) { /* remember the node the core made for this instance (identity only: no reference is kept) */
        int e = 0;
        VSNode *o = vs->mapGetNode(out, "clip", 0, &e);
        if (o && !e) { analyse_register(o, d); vs->freeNode(o); }
    }
}

/* ------------------------------------------------------------------------------------------------ mv.Finest */

typedef struct FinestData { VSNode *super; VSVideoInfo vi; mvx_super *sup; SuperGeo geo; ptrdiff_t pitch[3]; } FinestData;

static const VSFrame *VS_CC finestGetFrame(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    FinestData *d = (FinestData *)inst;
    if (reason == arInitial) { vs->requestFrameFilter(n, d->super, ctx); return NULL; }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *ref = vs->getFrameFilter(n, d->super, ctx);
    VSFrame *dst = vs->newVideoFrame(&d->vi.format, d->vi.width, d->vi.height, ref, core);
    const int np = d->vi.format.numPlanes, bps = d->vi.format.bytesPerSample;
    DevRef ds;
    int rc = super_to_device(&ds, ref, &d->geo, vs);
    size_t off[3], total = 0;
    for (int p = 0; p < np; p++) { off[p] = total; total += (size_t)d->pitch[p] * vs->getFrameHeight(dst, p); }
    void *arena = rc ? NULL : mvx_dev_alloc(total);
    if (!rc && !arena) rc = MVX_E_NOMEM;
    if (!rc) {
        const void *src3[3]; void *dst3[3];
        for (int p = 0; p < 3; p++) { src3[p] = ds.plane[p]; dst3[p] = p < np ? (char *)arena + off[p] : NULL; }
        rc = mvx_finest_frames(d->sup, 1, src3, d->geo.pitch, dst3, d->pitch, thread_stream());
        for (int p = 0; p < np && !rc; p++)
            rc = timed_download(vs->getWritePtr(dst, p), vs->getStride(dst, p), dst3[p], d->pitch[p], (size_t)vs->getFrameWidth(dst, p) * bps, (size_t)vs->getFrameHeight(dst, p));
        if (!rc) rc = mvx_stream_sync(thread_stream());
    }
    dev_release(&ds);
    shell_quiesce(rc);
    if (arena) mvx_dev_free(arena);
    vs->freeFrame(ref);
    if (rc) { vs->freeFrame(dst); vs->setFilterError(rc == MVX_E_NOMEM ? "Finest: out of memory." : mvx_last_error(), ctx); return NULL; }
    return dst;
}
static void VS_CC finestFree(void *inst, VSCore *core, const VSAPI *vs) {
    (void)core;
    FinestData *d = (FinestData *)inst;
    vs->freeNode(d->super); mvx_super_destroy(d->sup); free(d);
}
static void VS_CC finestCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    VSNode *super = vs->mapGetNode(in, "super", 0, 0);
    const VSVideoInfo *vi = vs->getVideoInfo(super);
    if (!super_format_ok(vi)) {
        vs->mapSetError(out, "Finest: input clip must be GRAY, 420, 422, 440, or 444, up to 16 bits, with constant dimensions.");
        vs->freeNode(super);
        return;
    }
    char err[1400] = "";
    mvx_super *sup = super_from_props(super, "Finest", err, sizeof(err), vs);
    if (!sup) { vs->mapSetError(out, err); vs->freeNode(super); return; }
    if (mvx_super_is_float(sup)) { /* mvx_finest_frames' refusal (csrc/mvx_super.hip, "Finest: float super clips are not supported."), word for word and at creation: mvx_finest_size has
                                    * no way to fail.  tests/test_vs_float_shell.py holds the two texts together */
        vs->mapSetError(out, "Finest: float super clips are not supported.");
        mvx_super_destroy(sup); vs->freeNode(super);
        return;
    }
    FinestData *d = (FinestData *)calloc(1, sizeof(*d));
    d->super = super; d->sup = sup; d->vi = *vi;
    super_geo(&d->geo, sup);
    int32_t w, h;
    mvx_finest_size(sup, &w, &h);
    d->vi.width = w; d->vi.height = h;
    for (int p = 0; p < 3; p++) {
        const int pw = p ? w >> vi->format.subSamplingW : w;
        d->pitch[p] = ((ptrdiff_t)pw * vi->format.bytesPerSample + 255) / 256 * 256;
    }
    VSFilterDependency deps[1] = { { super, rpStrictSpatial } };
    vs->createVideoFilter(out, "Finest", &d->vi, finestGetFrame, finestFree, fmParallel, deps, 1, d, core);
}

/* ------------------------------------------------------------------------------------------------ mv.SCDetection */

typedef struct ScdData { VSNode *node, *vectors; const VSVideoInfo *vi; mvx_analysis_data ad; int64_t thscd1; int32_t thscd2; } ScdData;

static const VSFrame *VS_CC scdGetFrame(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    ScdData *d = (ScdData *)inst;
    if (reason == arInitial) { vs->requestFrameFilter(n, d->vectors, ctx); vs->requestFrameFilter(n, d->node, ctx); return NULL; }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    VSFrame *dst = vs->copyFrame(src, core);
    vs->freeFrame(src);
    const VSFrame *mvn = vs->getFrameFilter(n, d->vectors, ctx);
    void *dblob = NULL;
    int rc = blob_to_device(&dblob, NULL, &d->ad, mvn, vs);
    vs->freeFrame(mvn);
    int32_t sc = 0;
    char lerr[MVX_ERRLEN];
    if (!rc) { const void *b1[1] = { dblob }; rc = mvx_scdetect(&d->ad, d->thscd1, d->thscd2, 1, b1, &sc, thread_stream(), lerr); }
    shell_quiesce(rc);
    if (dblob) mvx_dev_free(dblob);
    if (rc) { vs->freeFrame(dst); vs->setFilterError(rc == MVX_E_ARG ? "SCDetection: vector clip frame without a valid MVTools_vectors property." : mvx_last_error(), ctx); return NULL; }
    vs->mapSetInt(vs->getFramePropertiesRW(dst), d->ad.isBackward ? "_SceneChangeNext" : "_SceneChangePrev", sc, maReplace); /* :62-64 */
    return dst;
}
static void VS_CC scdFree(void *inst, VSCore *core, const VSAPI *vs) {
    (void)core;
    ScdData *d = (ScdData *)inst;
    vs->freeNode(d->node); vs->freeNode(d->vectors); free(d);
}
static void VS_CC scdCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    ScdData *d = (ScdData *)calloc(1, sizeof(*d));
    char err[1400] = "";
    d->thscd1 = opt_int64(in, "thscd1", vs); d->thscd2 = opt_int(in, "thscd2", vs);
    d->vectors = vs->mapGetNode(in, "vectors", 0, NULL);
    adata_from_clip(&d->ad, d->vectors, "SCDetection", "vectors", err, sizeof(err), vs);
    if (!err[0] && (d->thscd1 == (int64_t)MVX_UNSET ? 400 : d->thscd1) > 8 * 8 * 255) snprintf(err, sizeof(err), "SCDetection: thscd1 can be at most %d.", 8 * 8 * 255);
    if (err[0]) { vs->mapSetError(out, err); vs->freeNode(d->vectors); free(d); return; }
    d->node = vs->mapGetNode(in, "clip", 0, NULL);
    d->vi = vs->getVideoInfo(d->node);
    VSFilterDependency deps[2] = { { d->node, rpStrictSpatial }, { d->vectors, rpStrictSpatial } };
    vs->createVideoFilter(out, "SCDetection", d->vi, scdGetFrame, scdFree, fmParallel, deps, 2, d, core);
}

/* ------------------------------------------------------------------------------------------------ mv.Recalculate */

typedef struct RecalcData { VSNode *node, *vectors; const VSVideoInfo *vi; mvx_super *sup; SuperGeo geo; mvx_recalculate *rc; mvx_analysis_data ad, old; int blobSize; FieldOpt fo; } RecalcData;

static int recalc_nref(const RecalcData *d, int n) { /* src/MVRecalculate.c:78-85 */
    const int off = d->ad.nDeltaFrame;
    if (off > 0) return d->ad.isBackward ? n + off : n - off;
    return -off;
}

static const VSFrame *VS_CC recalcGetFrame(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    RecalcData *d = (RecalcData *)inst;
    const int nref = recalc_nref(d, n);
    const int haveRef = nref >= 0 && nref < d->vi->numFrames;
    if (reason == arInitial) {
        vs->requestFrameFilter(n, d->vectors, ctx);
        if (haveRef && nref < n) vs->requestFrameFilter(nref, d->node, ctx);
        vs->requestFrameFilter(n, d->node, ctx);
        if (haveRef && nref > n) vs->requestFrameFilter(nref, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    const VSFrame *ref = haveRef ? vs->getFrameFilter(nref, d->node, ctx) : NULL;
    if (d->fo.fields) { /* src/MVRecalculate.c:121-163: only the error survives, the shift itself never reaches a result */
        int missing = 0;
        frame_top_field(&d->fo, src, n, &missing, vs);
        if (ref) frame_top_field(&d->fo, ref, nref, &missing, vs);
        if (missing) {
            vs->setFilterError("Recalculate: _Field property not found in input frame. Therefore, you must pass tff argument.", ctx);
            if (ref) vs->freeFrame(ref);
            vs->freeFrame(src);
            return NULL;
        }
    }
    const VSFrame *mvn = vs->getFrameFilter(n, d->vectors, ctx);
    DevRef ds, dr;
    memset(&dr, 0, sizeof(dr));
    void *oldBlob = NULL;
    int rc = blob_to_device(&oldBlob, NULL, &d->old, mvn, vs);
    vs->freeFrame(mvn);
    if (!rc) rc = super_to_device(&ds, src, &d->geo, vs); else memset(&ds, 0, sizeof(ds));
    if (!rc && ref) rc = super_to_device(&dr, ref, &d->geo, vs);
    void *dblob = rc ? NULL : mvx_dev_alloc((size_t)d->blobSize);
    char *blob = (char *)malloc((size_t)d->blobSize);
    if (!rc && (!dblob || !blob)) rc = MVX_E_NOMEM;
    if (!rc) {
        mvx_recalculate_job job;
        memset(&job, 0, sizeof(job));
        for (int p = 0; p < 3; p++) { job.src[p] = ds.plane[p]; job.ref[p] = ref ? dr.plane[p] : NULL; }
        job.old_blob = oldBlob; job.blob = dblob;
        rc = mvx_recalculate_frames(d->rc, 1, &job, thread_stream());
        if (!rc) rc = timed_download(blob, d->blobSize, dblob, d->blobSize, (size_t)d->blobSize, 1);
        if (!rc) rc = mvx_stream_sync(thread_stream());
    }
    shell_quiesce(rc);
    dev_release(&ds); dev_release(&dr);
    if (dblob) mvx_dev_free(dblob);
    if (oldBlob) mvx_dev_free(oldBlob);
    if (ref) vs->freeFrame(ref);
    VSFrame *dst = NULL;
    if (!rc) { /* src/MVRecalculate.c:218-235 */
        dst = vs->copyFrame(src, core);
        VSMap *props = vs->getFramePropertiesRW(dst);
        vs->mapSetData(props, PROP_ADATA, (const char *)&d->ad, sizeof(d->ad), dtBinary, maReplace);
        vs->mapSetData(props, PROP_VECTORS, blob, d->blobSize, dtBinary, maReplace);
    } else
        vs->setFilterError(rc == MVX_E_ARG ? "Recalculate: vector clip frame without a valid MVTools_vectors property." : rc == MVX_E_NOMEM ? "Recalculate: out of memory." : mvx_last_error(), ctx);
    free(blob);
    vs->freeFrame(src);
    return dst;
}

static void VS_CC recalcFree(void *inst, VSCore *core, const VSAPI *vs) {
    (void)core;
    RecalcData *d = (RecalcData *)inst;
    vs->freeNode(d->node); vs->freeNode(d->vectors);
    mvx_recalculate_destroy(d->rc);
    mvx_super_destroy(d->sup);
    free(d);
}

static void VS_CC recalcCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    static const char *keys[] = { "thsad", "smooth", "blksize", "blksizev", "search", "searchparam", "lambda", "chroma", "truemotion", "pnew", "overlap", "overlapv",
                                  "divide", "meander", "fields", "dct" };
    mvx_recalculate_args a;
    int64_t *av = (int64_t *)&a;
    for (size_t i = 0; i < sizeof(keys) / sizeof(keys[0]); i++) av[i] = opt_int64(in, keys[i], vs);
    RecalcData *d = (RecalcData *)calloc(1, sizeof(*d));
    char err[1400] = "";
    field_opt(&d->fo, in, vs);
    d->node = vs->mapGetNode(in, "super", 0, 0);
    d->vi = vs->getVideoInfo(d->node);
    d->sup = super_from_props(d->node, "Recalculate", err, sizeof(err), vs);
    if (!err[0]) { d->vectors = vs->mapGetNode(in, "vectors", 0, NULL); adata_from_clip(&d->old, d->vectors, "Recalculate", "vectors", err, sizeof(err), vs); }
    if (!err[0]) {
        super_geo(&d->geo, d->sup);
        char lerr[MVX_ERRLEN];
        if (mvx_recalculate_create(&a, d->sup, &d->old, d->geo.pitch, &d->rc, lerr)) snprintf(err, sizeof(err), "%s", lerr);
    }
    if (err[0]) {
        vs->mapSetError(out, err);
        if (d->node) vs->freeNode(d->node);
        if (d->vectors) vs->freeNode(d->vectors);
        if (d->sup) mvx_super_destroy(d->sup);
        free(d);
        return;
    }
    mvx_recalculate_get_data(d->rc, &d->ad);
    d->blobSize = mvx_recalculate_blob_size(d->rc);
    VSFilterDependency deps[2] = { { d->node, rpGeneral }, { d->vectors, rpStrictSpatial } };
    vs->createVideoFilter(out, "Recalculate", d->vi, recalcGetFrame, recalcFree, fmParallel, deps, 2, d, core);
}

/* ------------------------------------------------------------------------------------------------ admission gate of the consuming filters (r6)
 * A host asks for as many output frames at once as it has worker threads -- a VapourSynth core starts one per logical CPU, 256 on the bench box.  Every output frame
 * in flight pins its 2 * radius + 1 super frames and pulls the look-ahead windows of the vector clips forward; past ~3/4 of a look-ahead window of frames in flight the
 * requests span three windows, the device cache turns over and 640 4K16 frames take 3.8-5.2 s (128 threads), 7-9.6 s (192) or 12-14 s (256) instead of 2.5 s (96):
 * profiles/r6_vs_shell_threads_96_to_256.txt.  So mv.DegrainN / mv.Compensate / mv.BlockFPS admit at most MVX_VS_MAX_INFLIGHT (default 96) of their own output frames
 * at a time, the lowest frame numbers first; a request beyond that waits at arInitial -- before it has asked for anything -- until an admitted frame is delivered or
 * fails.  The permit travels in the request's frame data (*fd), so arAllFramesReady / arError of the same request give it back.  One gate per filter instance: a chain of
 * such filters cannot deadlock on a shared pool. */
typedef struct GateWaiter { int n; pthread_cond_t cv; } GateWaiter; /* (one condition variable per waiter: a delivered frame wakes the ONE request it admits, not all of them) */
typedef struct Gate { pthread_mutex_t mu; int limit, inflight, nwait; long done; GateWaiter *waiting[1024]; } Gate;
static void gate_init(Gate *g) {
    pthread_mutex_init(&g->mu, NULL);
    g->limit = (int)env_long("MVX_VS_MAX_INFLIGHT", 96); /* (<= 0: no gate) */
    g->inflight = g->nwait = 0; g->done = 0;
}
static void gate_free(Gate *g) {
    if (g->inflight || g->nwait) fprintf(stderr, "mvtools_vs: admission gate freed with %d permits out, %d requests waiting\n", g->inflight, g->nwait); /* (a request that never ended: a bug here or in the host) */
    pthread_mutex_destroy(&g->mu);
}
static GateWaiter *gate_lowest(const Gate *g) { /* mu held */
    GateWaiter *w = NULL;
    for (int i = 0; i < g->nwait; i++) if (!w || g->waiting[i]->n < w->n) w = g->waiting[i];
    return w;
}
/* A waiter occupies one of the host's worker threads.  A host that has more requests outstanding than workers could end up with every worker waiting here and none
 * left for the upstream filters of the admitted frames; so the waiter that is next in line and sees NO admitted frame finish for a quarter of a second -- frames take
 * milliseconds -- goes on over the limit: slow, as without the gate, never stuck. */
static void gate_enter(Gate *g, int n, void **fd) {
    if (g->limit <= 0 || *fd) return;
    pthread_mutex_lock(&g->mu);
    if ((g->inflight >= g->limit || g->nwait) && g->nwait < 1024) {
        GateWaiter me;
        me.n = n;
        pthread_cond_init(&me.cv, NULL);
        g->waiting[g->nwait++] = &me;
        for (;;) {
            const int lowest = gate_lowest(g) == &me;
            if (g->inflight < g->limit && lowest) break;
            struct timespec ts;
            clock_gettime(CLOCK_REALTIME, &ts);
            ts.tv_nsec += 250000000L;
            if (ts.tv_nsec >= 1000000000L) { ts.tv_nsec -= 1000000000L; ts.tv_sec++; }
            const long seen = g->done;
            const int rc = pthread_cond_timedwait(&me.cv, &g->mu, &ts);
            if (rc == ETIMEDOUT && gate_lowest(g) == &me && g->done == seen) break;
        }
        for (int i = 0; i < g->nwait; i++) if (g->waiting[i] == &me) { g->waiting[i] = g->waiting[--g->nwait]; break; }
        pthread_cond_destroy(&me.cv);
        g->inflight++;
        if (g->inflight < g->limit && g->nwait) pthread_cond_signal(&gate_lowest(g)->cv); /* (room for the next one too) */
    } else g->inflight++;
    *fd = (void *)g;
    pthread_mutex_unlock(&g->mu);
}
static void gate_leave(Gate *g, void **fd) {
    if (!*fd) return;
    *fd = NULL;
    pthread_mutex_lock(&g->mu);
    g->inflight--; g->done++;
    if (g->nwait && g->inflight < g->limit) pthread_cond_signal(&gate_lowest(g)->cv);
    pthread_mutex_unlock(&g->mu);
}

/* ------------------------------------------------------------------------------------------------ the consuming filters: one skeleton
 * mv.Degrain1..6 / mv.Compensate / mv.BlockFPS and, registered with MVX_VS_FLOW=1 (see the entry point), mv.FlowInter / mv.FlowFPS / mv.Flow / mv.FlowBlur / mv.Mask
 * take vectors and produce pictures behind the admission gate.  Each has a Consumer as the FIRST member of its data: what an instance owns, the gate around its
 * getFrame and its free callback exist once.  Where the reference asks its mv.Finest node for a frame the per-sample filters ask the super clip: the library reads
 * the sub-pel planes of the super frame directly (mvtools_amd.h), so no Finest node exists.  One mvx_*_frames call per output frame, on the thread's stream. */
typedef struct Consumer {
    const char *name;
    Gate gate;
    VSNode *nodes[14]; int nnodes;         /* every node the instance holds (the filters' own node members point into this) */
    mvx_super *sup; SuperGeo geo;          /* of the super clip (mv.Mask takes none) */
    int floatEntry;                        /* the library has a *_create_float for this filter, which a float `clip` selects (MVX_VS_FLOAT=1) */
    void *engine; void (*destroy)(void *); /* the library's handle */
    VSFilterGetFrame body;                 /* the filter proper */
} Consumer;

#define ENGINE_DESTROY(T) static void T##_destroy_engine(void *e) { T##_destroy((T *)e); }
ENGINE_DESTROY(mvx_degrain) ENGINE_DESTROY(mvx_compensate) ENGINE_DESTROY(mvx_blockfps) ENGINE_DESTROY(mvx_flow) ENGINE_DESTROY(mvx_flowcomp) ENGINE_DESTROY(mvx_flowblur) ENGINE_DESTROY(mvx_mask)

static void *consumer_new(size_t size, const char *name, VSFilterGetFrame body, void (*destroy)(void *)) {
    Consumer *c = (Consumer *)calloc(1, size);
    c->name = name; c->body = body; c->destroy = destroy;
    gate_init(&c->gate);
    return c;
}
static VSNode *consumer_node(Consumer *c, const VSMap *in, const char *key, const VSAPI *vs) {
    return c->nodes[c->nnodes++] = vs->mapGetNode(in, key, 0, NULL);
}
static VSNode *consumer_super(Consumer *c, const VSMap *in, char *err, size_t esz, const VSAPI *vs) {
    VSNode *super = consumer_node(c, in, "super", vs);
    c->sup = super_from_props(super, c->name, err, esz, vs);
    if (c->sup) super_geo(&c->geo, c->sup);
    return super;
}
/* the admission gate around the filter proper: arInitial takes the permit, whatever ends the request -- the frame, a filter error, arError -- returns it */
static const VSFrame *VS_CC consumerGetFrame(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    Consumer *c = (Consumer *)inst;
    if (reason == arInitial) gate_enter(&c->gate, n, fd);
    const VSFrame *f = c->body(n, reason, inst, fd, ctx, core, vs);
    if (reason != arInitial || f) gate_leave(&c->gate, fd);
    return f;
}
/* the free callback, and the teardown of an instance whose creation failed part of the way (no permit can be out then) */
static void VS_CC consumerFree(void *inst, VSCore *core, const VSAPI *vs) {
    (void)core;
    Consumer *c = (Consumer *)inst;
    for (int i = 0; i < c->nnodes; i++) if (c->nodes[i]) vs->freeNode(c->nodes[i]);
    if (c->engine) c->destroy(c->engine);
    if (c->sup) mvx_super_destroy(c->sup);
    gate_free(&c->gate);
    free(c);
}
static void consumer_fail(Consumer *c, const char *err, VSMap *out, const VSAPI *vs) {
    vs->mapSetError(out, err);
    consumerFree(c, NULL, vs);
}

/* device pitches of clip and output planes: rows of 256 bytes */
static void clip_pitches(ptrdiff_t pitch[3], const VSVideoInfo *vi, int bps) {
    for (int p = 0; p < 3; p++) {
        const int w = p ? vi->width >> vi->format.subSamplingW : vi->width;
        pitch[p] = ((ptrdiff_t)w * bps + 255) / 256 * 256;
    }
}
/* The two tests of `clip` at creation; the first that fails writes its message.  The format test is the reference's (MVDegrains.cpp:693, MVCompensate.c:543,
 * MVBlockFPS.c:928, MVFlowInter.c:644, MVFlowFPS.c:794, MVFlow.cpp:526, MVFlowBlur.c:514).  Of the other, the reference has the sizes only (MVDegrains.cpp:683,
 * MVCompensate.c:535, MVBlockFPS.c:913-920): the kernels address the clip's planes with the vector clip's geometry and the super clip's sample size, which creation
 * ties to the super clip's, so a clip of another size or format than the one the super clip was made from would be read or written outside its planes. */
static void consumer_check_clip(const Consumer *c, const VSVideoInfo *vi, const VSVideoInfo *svi, int sizeFirst, char *err, size_t esz) {
    const mvx_super_info *si = &c->geo.si;
    /* MVX_VS_FLOAT=1: a float clip passes the format test of a filter that has a float entry in the library (c->floatEntry; the caller picks the entry by the clip's sample
     * type); the size test compares the sample types as well.  Where the entry the caller is about to use and the super clip disagree -- the float entry with an integer
     * super clip, an integer entry with a float one -- both tests are left out: that entry refuses the super clip whatever else it is given ("the float entry needs a float
     * super clip." / "float super clips are not supported."), so no instance exists whose planes the size test has not tied to the super clip's */
    const int floatClip = c->floatEntry && vi_is_float(vi);
    if (floatClip != mvx_super_is_float(c->sup)) return;
    const int formatOk = floatClip ? super_format_ok(vi) : integer_format_ok(vi);
    const int isSupers = si->width == vi->width && si->height == vi->height && si->super_width == svi->width && si->super_height == svi->height &&
                         vi->format.bitsPerSample == svi->format.bitsPerSample && vi->format.sampleType == svi->format.sampleType && vi->format.colorFamily == svi->format.colorFamily &&
                         vi->format.subSamplingW == svi->format.subSamplingW && vi->format.subSamplingH == svi->format.subSamplingH;
    if (!isSupers && (sizeFirst || formatOk)) snprintf(err, esz, "%s: wrong source or super clip frame size.", c->name);
    else if (!formatOk) snprintf(err, esz, "%s: input clip must be GRAY, 420, 422, 440, or 444, up to 16 bits, with constant dimensions.", c->name);
}
/* one arena for the planes of an output frame */
static int dst_plane_set(void *dst[3], void **arena, const ptrdiff_t pitch[3], const int height[3], int nplanes) {
    size_t off[3], total = 0;
    for (int p = 0; p < nplanes; p++) { off[p] = total; total += (size_t)pitch[p] * (size_t)height[p]; }
    for (int p = 0; p < 3; p++) dst[p] = NULL;
    *arena = shell_alloc(total);
    if (!*arena) return MVX_E_NOMEM;
    for (int p = 0; p < nplanes; p++) dst[p] = (char *)*arena + off[p];
    return 0;
}
/* the finished planes -> the host frame; complete on return */
static int download_plane_set(VSFrame *dst, void *const src[3], const ptrdiff_t pitch[3], int nplanes, int bps, const VSAPI *vs) {
    int rc = 0;
    for (int p = 0; p < nplanes && !rc; p++)
        rc = timed_download(vs->getWritePtr(dst, p), vs->getStride(dst, p), src[p], pitch[p], (size_t)vs->getFrameWidth(dst, p) * bps, (size_t)vs->getFrameHeight(dst, p));
    if (!rc) rc = mvx_stream_sync(thread_stream());
    return rc;
}
/* prefixAll: the library's own message gets the filter's name in front as well (mv.DegrainN's habit) */
static void consumer_frame_error(const char *name, int rc, int prefixAll, VSFrameContext *ctx, const VSAPI *vs) {
    char msg[MVX_ERRLEN + 64];
    if (rc != MVX_E_ARG && rc != MVX_E_NOMEM && !prefixAll) { vs->setFilterError(mvx_last_error(), ctx); return; }
    snprintf(msg, sizeof(msg), "%s: %s", name, rc == MVX_E_ARG ? "vector clip frame without matching MVTools_vectors property." : rc == MVX_E_NOMEM ? "out of memory." : mvx_last_error());
    vs->setFilterError(msg, ctx);
}
static double opt_float(const VSMap *in, const char *key, double def, const VSAPI *vs) {
    int e = 0;
    const double v = vs->mapGetFloat(in, key, 0, &e);
    return e ? def : v;
}
/* MVTools_vectors of frame n of a vector clip -> device; 0 or an MVX_E_* code */
static int clip_blob_to_device(void **dblob, int n, VSNode *vectors, const mvx_analysis_data *ad, VSFrameContext *ctx, const VSAPI *vs) {
    const VSFrame *vf = vs->getFrameFilter(n, vectors, ctx);
    const int rc = blob_to_device(dblob, NULL, ad, vf, vs);
    vs->freeFrame(vf);
    return rc;
}
static int clip_super_to_device(DevRef *r, int n, VSNode *super, const SuperGeo *g, VSFrameContext *ctx, const VSAPI *vs) {
    const VSFrame *sf = vs->getFrameFilter(n, super, ctx);
    const int rc = super_to_device(r, sf, g, vs);
    vs->freeFrame(sf);
    return rc;
}
/* mv.BlockFPS / mv.FlowFPS: AssumeFPS sets the _DurationNum / _DurationDen frame properties (src/MVBlockFPS.c:989-1014, src/MVFlowFPS.c:881-900) */
static void assume_fps(VSMap *out, const char *name, int64_t num, int64_t den, VSCore *core, const VSAPI *vs) {
    VSNode *node = vs->mapGetNode(out, "clip", 0, NULL);
    VSMap *args = vs->createMap();
    vs->mapSetNode(args, "clip", node, maReplace);
    vs->freeNode(node);
    vs->mapSetInt(args, "fpsnum", num, maReplace);
    vs->mapSetInt(args, "fpsden", den, maReplace);
    VSPlugin *std = vs->getPluginByID("com.vapoursynth.std", core);
    VSMap *ret = vs->invoke(std, "AssumeFPS", args);
    vs->freeMap(args);
    if (vs->mapGetError(ret)) {
        char msg[600];
        snprintf(msg, sizeof(msg), "%s: Failed to invoke AssumeFPS. Error message: %s", name, vs->mapGetError(ret));
        vs->mapSetError(out, msg);
        vs->freeMap(ret);
        return;
    }
    node = vs->mapGetNode(ret, "clip", 0, NULL);
    vs->freeMap(ret);
    vs->mapSetNode(out, "clip", node, maReplace);
    vs->freeNode(node);
}

/* ------------------------------------------------------------------------------------------------ mv.Degrain1..6 */

typedef struct DegrainData {
    Consumer c;
    VSNode *node, *super, *vectors[12];
    const VSVideoInfo *vi;
    int radius;
    mvx_degrain *dg;
    mvx_analysis_data ad[12];
    AnalyseData *an[12]; /* the mv.Analyse instances behind the vector clips, where they are this plugin's (r6: their vectors are read on the device) */
    ptrdiff_t pitch[3]; /* device pitch of clip / output planes */
} DegrainData;

typedef struct FirstFrameReq { const VSAPI *vs; VSNode *node; } FirstFrameReq;
static void *first_frame_thread(void *arg) { /* (errors are reported by the caller's own read of the frame) */
    FirstFrameReq *q = (FirstFrameReq *)arg;
    char msg[256];
    const VSFrame *f = q->vs->getFrame(0, q->node, msg, sizeof(msg));
    if (f) q->vs->freeFrame(f);
    return NULL;
}

static const VSFrame *VS_CC degrainGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    DegrainData *d = (DegrainData *)inst;
    const int nr = 2 * d->radius;
    if (reason == arInitial) { /* src/MVDegrains.cpp:92-109 */
        for (int r = 0; r < nr; r += 2) {
            vs->requestFrameFilter(n, d->vectors[r], ctx);
            vs->requestFrameFilter(n, d->vectors[r + 1], ctx);
            const int offB = d->ad[r].nDeltaFrame, offF = -d->ad[r + 1].nDeltaFrame;
            if (n + offB < d->vi->numFrames) vs->requestFrameFilter(n + offB, d->super, ctx);
            if (n + offF >= 0) vs->requestFrameFilter(n + offF, d->super, ctx);
        }
        vs->requestFrameFilter(n, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const double tgf = prof_now();
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    const int np = d->vi->format.numPlanes, bps = d->vi->format.bytesPerSample;
    mvx_degrain_job job;
    memset(&job, 0, sizeof(job));
    DevRef refs[12];
    void *blobArena[12];
    LaWindow *blobHeld[12];
    memset(refs, 0, sizeof(refs)); memset(blobArena, 0, sizeof(blobArena)); memset(blobHeld, 0, sizeof(blobHeld));
    void *srcArena = NULL, *dstArena = NULL, *dsrc[3], *ddst[3];
    int height[3] = { 0, 0, 0 };
    for (int p = 0; p < np; p++) height[p] = vs->getFrameHeight(src, p);
    int rc = upload_plane_set(dsrc, &srcArena, src, d->pitch, np, bps, vs);
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->pitch, height, np);
    for (int p = 0; p < np && !rc; p++) { job.src[p] = dsrc[p]; job.dst[p] = ddst[p]; }
    for (int r = 0; r < nr && !rc; r++) {
        const void *onDevice = la_device_blob(d->an[r] ? &d->an[r]->la : NULL, n, &blobHeld[r]);
        if (onDevice) job.blobs[r] = (void *)onDevice; /* (the window that made the frame's property: the same bytes) */
        else {
            rc = clip_blob_to_device(&blobArena[r], n, d->vectors[r], &d->ad[r], ctx, vs);
            job.blobs[r] = blobArena[r];
        }
        const int nref = (r & 1) ? n - d->ad[r].nDeltaFrame : n + d->ad[r].nDeltaFrame;
        if (!rc && nref >= 0 && nref < d->vi->numFrames) {
            rc = clip_super_to_device(&refs[r], nref, d->super, &d->c.geo, ctx, vs);
            for (int p = 0; p < 3; p++) job.refs[r][p] = refs[r].plane[p];
        }
    }
    const double tdg = prof_now();
    if (!rc) rc = mvx_degrain_frames(d->dg, 1, &job, thread_stream());
    if (!rc) rc = mvx_stream_sync(thread_stream());
    prof_add(PF_DEGRAIN, tdg);
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi->format, d->vi->width, d->vi->height, src, core);
        for (int p = 0; p < np && !rc; p++) /* (the kernels were waited for above: the download stream, beside the other threads' uploads) */
            rc = timed_download_on(download_stream(), vs->getWritePtr(dst, p), vs->getStride(dst, p), job.dst[p], d->pitch[p], (size_t)vs->getFrameWidth(dst, p) * bps, (size_t)vs->getFrameHeight(dst, p));
    }
    shell_quiesce(rc);
    for (int r = 0; r < nr; r++) { dev_release(&refs[r]); if (blobArena[r]) mvx_dev_free(blobArena[r]); if (blobHeld[r]) la_device_blob_release(&d->an[r]->la, blobHeld[r]); }
    if (srcArena) mvx_dev_free(srcArena);
    if (dstArena) mvx_dev_free(dstArena);
    vs->freeFrame(src);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error(d->c.name, rc, 1, ctx, vs);
        return NULL;
    }
    prof_add(PF_GF_DEGRAIN, tgf);
    if ((n & 31) == 0) la_trace(d, n, "(Degrain output frame of this number done)", prof_now() - tgf);
    return dst;
}

static void VS_CC degrainCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    const int radius = (int)(intptr_t)user;
    static const char *const names[] = { "Degrain1", "Degrain2", "Degrain3", "Degrain4", "Degrain5", "Degrain6" };
    static const char *vnames[] = { "mvbw", "mvfw", "mvbw2", "mvfw2", "mvbw3", "mvfw3", "mvbw4", "mvfw4", "mvbw5", "mvfw5", "mvbw6", "mvfw6" };
    DegrainData *d = (DegrainData *)consumer_new(sizeof(*d), names[radius - 1], degrainGetFrameUngated, mvx_degrain_destroy_engine);
    const char *name = d->c.name;
    d->radius = radius;
    char err[1400] = "";
    mvx_degrain_args a;
    a.radius = radius; a.thsad = opt_int64(in, "thsad", vs); a.thsadc = opt_int64(in, "thsadc", vs); a.plane = opt_int(in, "plane", vs);
    a.limit = opt_int(in, "limit", vs); a.limitc = opt_int(in, "limitc", vs); a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    if (a.plane != MVX_UNSET && (a.plane < 0 || a.plane > 4)) snprintf(err, sizeof(err), "%s: plane must be between 0 and 4 (inclusive).", name);
    if (!err[0]) d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    const int nr = 2 * radius;
    for (int r = 0; r < nr && !err[0]; r++) d->vectors[r] = consumer_node(&d->c, in, vnames[r], vs);
    if (!err[0] && env_long("MVX_VS_PARALLEL_FIRST", 1)) { /* r6: frame 0 of the vector clips is produced CONCURRENTLY (each is a whole look-ahead window of searches: six launches
                                                             * that share the GPU instead of queueing behind each other); the reads below then find the frames in the host's cache */
        pthread_t th[12];
        FirstFrameReq fr[12];
        int started[12];
        for (int r = 0; r < nr; r++) { fr[r].vs = vs; fr[r].node = d->vectors[r]; started[r] = pthread_create(&th[r], NULL, first_frame_thread, &fr[r]) == 0; }
        for (int r = 0; r < nr; r++) if (started[r]) pthread_join(th[r], NULL);
    }
    for (int r = 0; r < nr && !err[0]; r++) adata_from_clip(&d->ad[r], d->vectors[r], name, vnames[r], err, sizeof(err), vs);
    for (int r = 1; r < nr && !err[0]; r++) adata_similar(&d->ad[0], &d->ad[r], name, vnames[0], vnames[r], err, sizeof(err));
    if (!err[0]) { /* src/MVDegrains.cpp:606-640 */
        const char *m = NULL;
        for (int r = 0; r < nr; r++) if (d->ad[r].nDeltaFrame <= 0) m = "cannot use motion vectors with absolute frame references.";
        if (!d->ad[0].isBackward) m = "mvbw must be generated with isb=True.";
        if (d->ad[1].isBackward) m = "mvfw must be generated with isb=False.";
        for (int k = 1; k < radius; k++) {
            if (!d->ad[2 * k].isBackward) m = "mvbw must be generated with isb=True.";
            if (d->ad[2 * k + 1].isBackward) m = "mvfw must be generated with isb=False.";
            if (d->ad[2 * k].nDeltaFrame <= d->ad[2 * k - 2].nDeltaFrame) m = "mvbwN must have greater delta than mvbwP.";
            if (d->ad[2 * k + 1].nDeltaFrame <= d->ad[2 * k - 1].nDeltaFrame) m = "mvfwN must have greater delta than mvfwP.";
        }
        if (m) snprintf(err, sizeof(err), "%s: %s", name, m);
    }
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->vi = vs->getVideoInfo(d->node);
        consumer_check_clip(&d->c, d->vi, vs->getVideoInfo(d->super), 0, err, sizeof(err));
    }
    if (!err[0]) {
        clip_pitches(d->pitch, d->vi, d->vi->format.bytesPerSample);
        char lerr[MVX_ERRLEN];
        if (mvx_degrain_create(&a, &d->ad[0], d->c.sup, d->pitch, d->c.geo.pitch, d->pitch, &d->dg, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        else if (d->c.geo.copies > 1) mvx_degrain_set_ref_shadow(d->dg, d->c.geo.shadowStride); /* every device super frame of this shell carries its copies */
        d->c.engine = d->dg;
    }
    if (!err[0] && env_long("MVX_VS_DEVICE_VECTORS", 1)) for (int r = 0; r < nr; r++) d->an[r] = analyse_lookup(d->vectors[r]);
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    VSFilterDependency deps[14];
    deps[0].source = d->node; deps[0].requestPattern = rpStrictSpatial;
    deps[1].source = d->super; deps[1].requestPattern = rpGeneral;
    for (int r = 0; r < nr; r++) { deps[2 + r].source = d->vectors[r]; deps[2 + r].requestPattern = rpStrictSpatial; }
    vs->createVideoFilter(out, name, d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 2 + nr, d, core);
}

/* ------------------------------------------------------------------------------------------------ mv.Compensate */

typedef struct CompData { Consumer c; VSNode *node, *super, *vectors; const VSVideoInfo *vi; mvx_compensate *cp; mvx_analysis_data ad; ptrdiff_t pitch[3]; FieldOpt fo; } CompData;

static int comp_nref(const CompData *d, int n) { /* src/MVCompensate.c:84-92 */
    if (d->ad.nDeltaFrame > 0) return n + (d->ad.isBackward ? d->ad.nDeltaFrame : -d->ad.nDeltaFrame);
    return -d->ad.nDeltaFrame;
}

static const VSFrame *VS_CC compGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    CompData *d = (CompData *)inst;
    const int nref = comp_nref(d, n);
    const int haveRef = nref >= 0 && nref < d->vi->numFrames;
    if (reason == arInitial) {
        vs->requestFrameFilter(n, d->vectors, ctx);
        if (haveRef && nref < n) vs->requestFrameFilter(nref, d->super, ctx);
        vs->requestFrameFilter(n, d->super, ctx);
        if (haveRef && nref > n) vs->requestFrameFilter(nref, d->super, ctx);
        vs->requestFrameFilter(n, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    const VSFrame *ssup = vs->getFrameFilter(n, d->super, ctx);
    const VSFrame *rsup = haveRef ? vs->getFrameFilter(nref, d->super, ctx) : NULL;
    const VSFrame *vf = vs->getFrameFilter(n, d->vectors, ctx);
    const int np = d->vi->format.numPlanes, bps = d->vi->format.bytesPerSample;
    int fieldShift = 0;
    if (rsup && d->fo.fields && d->ad.nPel > 1 && ((nref - n) % 2 != 0)) { /* src/MVCompensate.c:188-225 (the props of the two super frames).
        * The reference only looks at _Field when the vectors are usable (:162); usability is decided on the device here, so a missing _Field is
        * reported for scene-change frames too. */
        int missing = 0;
        const int srcTop = frame_top_field(&d->fo, ssup, n, &missing, vs);
        const int refTop = frame_top_field(&d->fo, rsup, nref, &missing, vs);
        if (missing) {
            vs->setFilterError("Compensate: _Field property not found in input frame. Therefore, you must pass tff argument.", ctx);
            vs->freeFrame(vf); vs->freeFrame(ssup); vs->freeFrame(rsup); vs->freeFrame(src);
            return NULL;
        }
        fieldShift = field_shift_of(srcTop, refTop, d->ad.nPel);
    }
    DevRef ds, dr;
    memset(&dr, 0, sizeof(dr));
    int rc = super_to_device(&ds, ssup, &d->c.geo, vs);
    if (!rc && rsup) rc = super_to_device(&dr, rsup, &d->c.geo, vs);
    void *dblob = NULL, *dstArena = NULL, *ddst[3];
    if (!rc) rc = blob_to_device(&dblob, NULL, &d->ad, vf, vs);
    int height[3] = { 0, 0, 0 };
    for (int p = 0; p < np; p++) height[p] = vs->getFrameHeight(src, p);
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->pitch, height, np);
    mvx_compensate_job job;
    memset(&job, 0, sizeof(job));
    if (!rc) {
        for (int p = 0; p < 3; p++) { job.src_super[p] = ds.plane[p]; job.ref_super[p] = rsup ? dr.plane[p] : NULL; }
        for (int p = 0; p < np; p++) job.dst[p] = ddst[p];
        job.blob = dblob;
        job.field_shift = fieldShift;
        rc = mvx_compensate_frames(d->cp, 1, &job, thread_stream());
    }
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi->format, d->vi->width, d->vi->height, src, core);
        rc = download_plane_set(dst, ddst, d->pitch, np, bps, vs);
    }
    shell_quiesce(rc);
    dev_release(&ds); dev_release(&dr);
    if (dblob) mvx_dev_free(dblob);
    if (dstArena) mvx_dev_free(dstArena);
    vs->freeFrame(vf); vs->freeFrame(ssup); if (rsup) vs->freeFrame(rsup);
    vs->freeFrame(src);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error("Compensate", rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

static void VS_CC compCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    CompData *d = (CompData *)consumer_new(sizeof(*d), "Compensate", compGetFrameUngated, mvx_compensate_destroy_engine);
    char err[1400] = "";
    mvx_compensate_args a;
    a.scbehavior = opt_int(in, "scbehavior", vs); a.thsad = opt_int64(in, "thsad", vs); a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    a.time = opt_float(in, "time", 100.0, vs);
    field_opt(&d->fo, in, vs);
    a.fields = d->fo.fields;
    d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) { d->vectors = consumer_node(&d->c, in, "vectors", vs); adata_from_clip(&d->ad, d->vectors, "Compensate", "vectors", err, sizeof(err), vs); }
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->vi = vs->getVideoInfo(d->node);
        d->c.floatEntry = 1;
        consumer_check_clip(&d->c, d->vi, vs->getVideoInfo(d->super), 1, err, sizeof(err)); /* (the size first, as MVCompensate.c:535-545) */
    }
    if (!err[0]) {
        clip_pitches(d->pitch, d->vi, d->vi->format.bytesPerSample);
        char lerr[MVX_ERRLEN];
        if ((vi_is_float(d->vi) ? mvx_compensate_create_float : mvx_compensate_create)(&a, &d->ad, d->c.sup, d->c.geo.pitch, d->pitch, &d->cp, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        d->c.engine = d->cp;
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    VSFilterDependency deps[3] = { { d->node, rpStrictSpatial }, { d->super, rpGeneral }, { d->vectors, rpStrictSpatial } };
    vs->createVideoFilter(out, "Compensate", d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 3, d, core);
}

/* ------------------------------------------------------------------------------------------------ mv.BlockFPS */

typedef struct FpsData { Consumer c; VSNode *node, *super, *mvbw, *mvfw; const VSVideoInfo *oldvi; VSVideoInfo vi; mvx_blockfps *bf; mvx_analysis_data bw, fw; ptrdiff_t pitch[3]; } FpsData;

static int fps_min(int a, int b) { return a < b ? a : b; }

static const VSFrame *VS_CC fpsGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    FpsData *d = (FpsData *)inst;
    int nleft, nright, time256;
    mvx_blockfps_map(d->bf, n, &nleft, &nright, &time256);
    const int last = d->oldvi->numFrames - 1;
    const int good = nleft < d->oldvi->numFrames && nright < d->oldvi->numFrames;
    if (reason == arInitial) { /* src/MVBlockFPS.c:236-276 */
        if (time256 == 0) { vs->requestFrameFilter(fps_min(nleft, last), d->node, ctx); return NULL; }
        if (time256 == 256) { vs->requestFrameFilter(fps_min(nright, last), d->node, ctx); return NULL; }
        if (good) {
            vs->requestFrameFilter(nright, d->mvfw, ctx);
            vs->requestFrameFilter(nleft, d->mvbw, ctx);
            vs->requestFrameFilter(nleft, d->super, ctx);
            vs->requestFrameFilter(nright, d->super, ctx);
        }
        vs->requestFrameFilter(fps_min(nleft, last), d->node, ctx);
        vs->requestFrameFilter(fps_min(nright, last), d->node, ctx); /* the reference only asks for it when blend=1; harmless */
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    if (time256 == 0) return vs->getFrameFilter(fps_min(nleft, last), d->node, ctx);   /* simply left  (:285-286) */
    if (time256 == 256) return vs->getFrameFilter(fps_min(nright, last), d->node, ctx); /* simply right (:287-288) */
    const VSFrame *cl = vs->getFrameFilter(fps_min(nleft, last), d->node, ctx);
    const VSFrame *cr = vs->getFrameFilter(fps_min(nright, last), d->node, ctx);
    const int np = d->vi.format.numPlanes, bps = d->vi.format.bytesPerSample;
    mvx_blockfps_job job;
    memset(&job, 0, sizeof(job));
    job.time256 = time256;
    void *arenaL = NULL, *arenaR = NULL, *dstArena = NULL, *dl[3], *dr[3], *ddst[3], *blobF = NULL, *blobB = NULL;
    int height[3] = { 0, 0, 0 };
    for (int p = 0; p < np; p++) height[p] = vs->getFrameHeight(cl, p);
    int rc = upload_plane_set(dl, &arenaL, cl, d->pitch, np, bps, vs);
    if (!rc) rc = upload_plane_set(dr, &arenaR, cr, d->pitch, np, bps, vs);
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->pitch, height, np);
    for (int p = 0; p < np && !rc; p++) { job.clip_left[p] = dl[p]; job.clip_right[p] = dr[p]; job.dst[p] = ddst[p]; }
    DevRef ds, dr2;
    memset(&ds, 0, sizeof(ds)); memset(&dr2, 0, sizeof(dr2));
    if (!rc && good) {
        rc = clip_super_to_device(&ds, nleft, d->super, &d->c.geo, ctx, vs);
        if (!rc) rc = clip_super_to_device(&dr2, nright, d->super, &d->c.geo, ctx, vs);
        if (!rc) rc = clip_blob_to_device(&blobF, nright, d->mvfw, &d->fw, ctx, vs);
        if (!rc) rc = clip_blob_to_device(&blobB, nleft, d->mvbw, &d->bw, ctx, vs);
        for (int p = 0; p < 3; p++) { job.src_super[p] = ds.plane[p]; job.ref_super[p] = dr2.plane[p]; }
        job.blob_fw = blobF; job.blob_bw = blobB;
    }
    if (!rc) rc = mvx_blockfps_frames(d->bf, 1, &job, thread_stream());
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi.format, d->vi.width, d->vi.height, cl, core);
        rc = download_plane_set(dst, ddst, d->pitch, np, bps, vs);
    }
    shell_quiesce(rc);
    dev_release(&ds); dev_release(&dr2);
    if (blobF) mvx_dev_free(blobF);
    if (blobB) mvx_dev_free(blobB);
    if (arenaL) mvx_dev_free(arenaL);
    if (arenaR) mvx_dev_free(arenaR);
    if (dstArena) mvx_dev_free(dstArena);
    vs->freeFrame(cl); vs->freeFrame(cr);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error("BlockFPS", rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

static void VS_CC fpsCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    FpsData *d = (FpsData *)consumer_new(sizeof(*d), "BlockFPS", fpsGetFrameUngated, mvx_blockfps_destroy_engine);
    char err[1400] = "";
    mvx_blockfps_args a;
    a.num = opt_int64(in, "num", vs); a.den = opt_int64(in, "den", vs); a.mode = opt_int(in, "mode", vs); a.blend = opt_int(in, "blend", vs);
    a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    a.ml = opt_float(in, "ml", 100.0, vs);
    if (a.mode != MVX_UNSET && (a.mode < 0 || a.mode > 8)) snprintf(err, sizeof(err), "BlockFPS: mode must be between 0 and 8 (inclusive).");
    if (!err[0]) d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) { d->mvbw = consumer_node(&d->c, in, "mvbw", vs); adata_from_clip(&d->bw, d->mvbw, "BlockFPS", "mvbw", err, sizeof(err), vs); }
    if (!err[0]) { d->mvfw = consumer_node(&d->c, in, "mvfw", vs); adata_from_clip(&d->fw, d->mvfw, "BlockFPS", "mvfw", err, sizeof(err), vs); }
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->oldvi = vs->getVideoInfo(d->node);
        d->vi = *d->oldvi;
        clip_pitches(d->pitch, &d->vi, d->vi.format.bytesPerSample);
        char lerr[MVX_ERRLEN];
        d->c.floatEntry = 1;
        if ((vi_is_float(d->oldvi) ? mvx_blockfps_create_float : mvx_blockfps_create)(&a, &d->bw, &d->fw, d->c.sup, d->oldvi->numFrames, d->oldvi->fpsNum, d->oldvi->fpsDen, d->c.geo.pitch, d->pitch, d->pitch, &d->bf, lerr))
            snprintf(err, sizeof(err), "%s", lerr);
        else consumer_check_clip(&d->c, &d->vi, vs->getVideoInfo(d->super), 0, err, sizeof(err));
        d->c.engine = d->bf;
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    mvx_blockfps_info info;
    mvx_blockfps_get_info(d->bf, &info);
    d->vi.numFrames = info.num_frames; d->vi.fpsNum = info.fps_num; d->vi.fpsDen = info.fps_den;
    VSFilterDependency deps[4] = { { d->node, rpGeneral }, { d->super, rpGeneral }, { d->mvbw, rpGeneral }, { d->mvfw, rpGeneral } };
    vs->createVideoFilter(out, "BlockFPS", &d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 4, d, core);
    assume_fps(out, "BlockFPS", info.fps_num, info.fps_den, core, vs);
}

/* ------------------------------------------------------------------------------------------------ mv.FlowInter / mv.FlowFPS (one engine, one shell) */

typedef struct FlowData { Consumer c; VSNode *node, *super, *mvbw, *mvfw; const VSVideoInfo *oldvi; VSVideoInfo vi; mvx_flow *fl; mvx_analysis_data bw, fw; ptrdiff_t pitch[3];
                          int fps /* FlowFPS, else FlowInter */, extra /* the Extra formula's second pair of vectors is read */; } FlowData;

static const VSFrame *VS_CC flowGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    FlowData *d = (FlowData *)inst;
    int nleft, nright, time256;
    mvx_flow_map(d->fl, n, &nleft, &nright, &time256);
    const int last = d->oldvi->numFrames - 1;
    const int good = nleft <= last && nright <= last;
    const int ncl = fps_min(nleft, last), ncr = fps_min(nright, last);
    const int copies = d->fps && (time256 == 0 || time256 == 256); /* MVFlowFPS.c:101-107,138-142; FlowInter has no such shortcut */
    if (reason == arInitial) { /* src/MVFlowInter.c:86-102, src/MVFlowFPS.c:92-124 */
        if (copies) { vs->requestFrameFilter(time256 ? ncr : ncl, d->node, ctx); return NULL; }
        if (good) {
            if (d->extra) vs->requestFrameFilter(nleft, d->mvfw, ctx);
            vs->requestFrameFilter(nright, d->mvfw, ctx);
            vs->requestFrameFilter(nleft, d->mvbw, ctx);
            if (d->extra) vs->requestFrameFilter(nright, d->mvbw, ctx);
            vs->requestFrameFilter(nleft, d->super, ctx);
            vs->requestFrameFilter(nright, d->super, ctx);
        }
        vs->requestFrameFilter(ncl, d->node, ctx);
        vs->requestFrameFilter(ncr, d->node, ctx); /* FlowFPS only asks for it when blend=1; harmless */
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    if (copies) return vs->getFrameFilter(time256 ? ncr : ncl, d->node, ctx); /* simply left / right */
    const VSFrame *cl = vs->getFrameFilter(ncl, d->node, ctx);
    const VSFrame *cr = vs->getFrameFilter(ncr, d->node, ctx);
    const int np = d->vi.format.numPlanes, bps = d->vi.format.bytesPerSample;
    mvx_flow_job job;
    memset(&job, 0, sizeof(job));
    job.time256 = time256;
    void *arenaL = NULL, *arenaR = NULL, *dstArena = NULL, *dl[3], *dr[3], *ddst[3], *blob[4] = { NULL, NULL, NULL, NULL };
    int height[3] = { 0, 0, 0 };
    for (int p = 0; p < np; p++) height[p] = vs->getFrameHeight(cl, p);
    int rc = upload_plane_set(dl, &arenaL, cl, d->pitch, np, bps, vs);
    if (!rc) rc = upload_plane_set(dr, &arenaR, cr, d->pitch, np, bps, vs);
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->pitch, height, np);
    for (int p = 0; p < np && !rc; p++) { job.clip_left[p] = dl[p]; job.clip_right[p] = dr[p]; job.dst[p] = ddst[p]; }
    DevRef sl, sr;
    memset(&sl, 0, sizeof(sl)); memset(&sr, 0, sizeof(sr));
    if (!rc && good) { /* (else all four stay NULL: Blend or the left frame) */
        rc = clip_super_to_device(&sl, nleft, d->super, &d->c.geo, ctx, vs);
        if (!rc) rc = clip_super_to_device(&sr, nright, d->super, &d->c.geo, ctx, vs);
        if (!rc) rc = clip_blob_to_device(&blob[0], nright, d->mvfw, &d->fw, ctx, vs);
        if (!rc) rc = clip_blob_to_device(&blob[1], nleft, d->mvbw, &d->bw, ctx, vs);
        if (!rc && d->extra) rc = clip_blob_to_device(&blob[2], nleft, d->mvfw, &d->fw, ctx, vs);
        if (!rc && d->extra) rc = clip_blob_to_device(&blob[3], nright, d->mvbw, &d->bw, ctx, vs);
        for (int p = 0; p < 3; p++) { job.super_left[p] = sl.plane[p]; job.super_right[p] = sr.plane[p]; }
        job.blob_fw = blob[0]; job.blob_bw = blob[1]; job.blob_fw_extra = blob[2]; job.blob_bw_extra = blob[3];
    }
    if (!rc) rc = mvx_flow_frames(d->fl, 1, &job, thread_stream());
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi.format, d->vi.width, d->vi.height, cl, core);
        rc = download_plane_set(dst, ddst, d->pitch, np, bps, vs);
    }
    shell_quiesce(rc);
    dev_release(&sl); dev_release(&sr);
    for (int i = 0; i < 4; i++) if (blob[i]) mvx_dev_free(blob[i]);
    if (arenaL) mvx_dev_free(arenaL);
    if (arenaR) mvx_dev_free(arenaR);
    if (dstArena) mvx_dev_free(dstArena);
    vs->freeFrame(cl); vs->freeFrame(cr);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error(d->c.name, rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

/* user != NULL: mv.FlowFPS (src/MVFlowFPS.c:565-900), else mv.FlowInter (src/MVFlowInter.c:473-678) */
static void VS_CC flowCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    FlowData *d = (FlowData *)consumer_new(sizeof(*d), user ? "FlowFPS" : "FlowInter", flowGetFrameUngated, mvx_flow_destroy_engine);
    const char *name = d->c.name;
    d->fps = user != NULL;
    char err[1400] = "";
    mvx_flowinter_args ai;
    mvx_flowfps_args af;
    ai.time = opt_float(in, "time", 50.0, vs); ai.ml = af.ml = opt_float(in, "ml", 100.0, vs);
    ai.blend = af.blend = opt_int(in, "blend", vs);
    ai.thscd1 = af.thscd1 = opt_int64(in, "thscd1", vs); ai.thscd2 = af.thscd2 = opt_int(in, "thscd2", vs);
    af.num = opt_int64(in, "num", vs); af.den = opt_int64(in, "den", vs); af.mask = opt_int(in, "mask", vs);
    d->extra = d->fps ? (af.mask == MVX_UNSET || af.mask == 2) : 1;
    d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) { d->mvbw = consumer_node(&d->c, in, "mvbw", vs); adata_from_clip(&d->bw, d->mvbw, name, "mvbw", err, sizeof(err), vs); }
    if (!err[0]) { d->mvfw = consumer_node(&d->c, in, "mvfw", vs); adata_from_clip(&d->fw, d->mvfw, name, "mvfw", err, sizeof(err), vs); }
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->oldvi = vs->getVideoInfo(d->node);
        d->vi = *d->oldvi;
        clip_pitches(d->pitch, &d->vi, d->vi.format.bytesPerSample);
        char lerr[MVX_ERRLEN];
        const int flt = vi_is_float(d->oldvi);
        d->c.floatEntry = 1;
        const int rc = d->fps ? (flt ? mvx_flowfps_create_float : mvx_flowfps_create)(&af, &d->bw, &d->fw, d->c.sup, d->oldvi->numFrames, d->oldvi->fpsNum, d->oldvi->fpsDen, d->c.geo.pitch, d->pitch, d->pitch, &d->fl, lerr)
                              : (flt ? mvx_flowinter_create_float : mvx_flowinter_create)(&ai, &d->bw, &d->fw, d->c.sup, d->oldvi->numFrames, d->c.geo.pitch, d->pitch, d->pitch, &d->fl, lerr);
        if (rc) snprintf(err, sizeof(err), "%s", lerr);
        else consumer_check_clip(&d->c, &d->vi, vs->getVideoInfo(d->super), 0, err, sizeof(err));
        d->c.engine = d->fl;
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    VSFilterDependency deps[4] = { { d->node, rpGeneral }, { d->super, rpGeneral }, { d->mvbw, rpGeneral }, { d->mvfw, rpGeneral } };
    if (d->fps) { /* (mv.FlowInter's output clip is the input's) */
        mvx_flow_info info;
        mvx_flow_get_info(d->fl, &info);
        d->vi.numFrames = info.num_frames; d->vi.fpsNum = info.fps_num; d->vi.fpsDen = info.fps_den;
    }
    vs->createVideoFilter(out, name, &d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 4, d, core);
    if (d->fps) assume_fps(out, name, d->vi.fpsNum, d->vi.fpsDen, core, vs);
}

/* ------------------------------------------------------------------------------------------------ mv.Flow */

typedef struct FlowCompData { Consumer c; VSNode *node, *super, *vectors; const VSVideoInfo *vi; mvx_flowcomp *fc; mvx_analysis_data ad; ptrdiff_t pitch[3]; FieldOpt fo; } FlowCompData;

static const VSFrame *VS_CC flowCompGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    FlowCompData *d = (FlowCompData *)inst;
    const int nref = mvx_flowcomp_ref(d->fc, n);
    const int haveRef = nref >= 0 && nref < d->vi->numFrames;
    /* the parities of frames n and nref decide the field shift (src/MVFlow.cpp:264-297): only then is super frame n needed at all -- the reference always asks
     * for Finest frame n and reads nothing else from it */
    const int parity = haveRef && d->fo.fields && d->ad.nPel > 1 && ((nref - n) % 2 != 0);
    if (reason == arInitial) { /* src/MVFlow.cpp:170-192 */
        vs->requestFrameFilter(n, d->vectors, ctx);
        if (haveRef) {
            if (nref < n) vs->requestFrameFilter(nref, d->super, ctx);
            if (parity) vs->requestFrameFilter(n, d->super, ctx);
            if (nref >= n) vs->requestFrameFilter(nref, d->super, ctx);
        }
        vs->requestFrameFilter(n, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    const VSFrame *rsup = haveRef ? vs->getFrameFilter(nref, d->super, ctx) : NULL;
    const int np = d->vi->format.numPlanes, bps = d->vi->format.bytesPerSample;
    int fieldShift = 0;
    if (parity) { /* (as mv.Compensate here: usability is decided on the device, so a missing _Field is reported for scene-change frames too) */
        const VSFrame *ssup = vs->getFrameFilter(n, d->super, ctx);
        int missing = 0;
        const int srcTop = frame_top_field(&d->fo, ssup, n, &missing, vs);
        const int refTop = frame_top_field(&d->fo, rsup, nref, &missing, vs);
        vs->freeFrame(ssup);
        if (missing) {
            vs->setFilterError("Flow: _Field property not found in super frame. Therefore, you must pass tff argument.", ctx);
            vs->freeFrame(rsup); vs->freeFrame(src);
            return NULL;
        }
        fieldShift = field_shift_of(srcTop, refTop, d->ad.nPel);
    }
    mvx_flowcomp_job job;
    memset(&job, 0, sizeof(job));
    job.field_shift = fieldShift;
    void *srcArena = NULL, *dstArena = NULL, *dsrc[3], *ddst[3], *dblob = NULL;
    int height[3] = { 0, 0, 0 };
    for (int p = 0; p < np; p++) height[p] = vs->getFrameHeight(src, p);
    int rc = upload_plane_set(dsrc, &srcArena, src, d->pitch, np, bps, vs);
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->pitch, height, np);
    for (int p = 0; p < np && !rc; p++) { job.clip[p] = dsrc[p]; job.dst[p] = ddst[p]; }
    DevRef dr;
    memset(&dr, 0, sizeof(dr));
    if (!rc && rsup) rc = super_to_device(&dr, rsup, &d->c.geo, vs);
    if (!rc) rc = clip_blob_to_device(&dblob, n, d->vectors, &d->ad, ctx, vs);
    for (int p = 0; p < 3; p++) job.ref_super[p] = rsup ? dr.plane[p] : NULL; /* NULL: copy of the clip frame */
    job.blob = dblob;
    if (!rc) rc = mvx_flowcomp_frames(d->fc, 1, &job, thread_stream());
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi->format, d->vi->width, d->vi->height, src, core);
        rc = download_plane_set(dst, ddst, d->pitch, np, bps, vs);
    }
    shell_quiesce(rc);
    dev_release(&dr);
    if (dblob) mvx_dev_free(dblob);
    if (srcArena) mvx_dev_free(srcArena);
    if (dstArena) mvx_dev_free(dstArena);
    if (rsup) vs->freeFrame(rsup);
    vs->freeFrame(src);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error("Flow", rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

/* src/MVFlow.cpp:391-593 (fields=1 with pel=1 is accepted there and shifts nothing: :265) */
static void VS_CC flowCompCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    FlowCompData *d = (FlowCompData *)consumer_new(sizeof(*d), "Flow", flowCompGetFrameUngated, mvx_flowcomp_destroy_engine);
    char err[1400] = "";
    mvx_flowcomp_args a;
    a.time = opt_float(in, "time", 100.0, vs); a.mode = opt_int(in, "mode", vs);
    a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    field_opt(&d->fo, in, vs);
    a.fields = d->fo.fields;
    d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) { d->vectors = consumer_node(&d->c, in, "vectors", vs); adata_from_clip(&d->ad, d->vectors, "Flow", "vectors", err, sizeof(err), vs); }
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->vi = vs->getVideoInfo(d->node);
        clip_pitches(d->pitch, d->vi, d->vi->format.bytesPerSample);
        char lerr[MVX_ERRLEN];
        d->c.floatEntry = 1;
        if ((vi_is_float(d->vi) ? mvx_flowcomp_create_float : mvx_flowcomp_create)(&a, &d->ad, d->c.sup, d->vi->numFrames, d->c.geo.pitch, d->pitch, d->pitch, &d->fc, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        else consumer_check_clip(&d->c, d->vi, vs->getVideoInfo(d->super), 0, err, sizeof(err));
        d->c.engine = d->fc;
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    VSFilterDependency deps[3] = { { d->node, rpStrictSpatial }, { d->super, rpGeneral }, { d->vectors, rpStrictSpatial } };
    vs->createVideoFilter(out, "Flow", d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 3, d, core);
}

/* ------------------------------------------------------------------------------------------------ mv.FlowBlur */

typedef struct BlurData { Consumer c; VSNode *node, *super, *mvbw, *mvfw; const VSVideoInfo *vi; mvx_flowblur *fb; mvx_analysis_data bw, fw; ptrdiff_t pitch[3]; } BlurData;

static const VSFrame *VS_CC blurGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    BlurData *d = (BlurData *)inst;
    const int off = d->bw.nDeltaFrame;
    const int both = n - off >= 0 && n + off < d->vi->numFrames;
    if (reason == arInitial) { /* src/MVFlowBlur.c:148-157 */
        if (both) {
            vs->requestFrameFilter(n - off, d->mvbw, ctx);
            vs->requestFrameFilter(n + off, d->mvfw, ctx);
        }
        vs->requestFrameFilter(n, d->super, ctx);
        vs->requestFrameFilter(n, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    const int np = d->vi->format.numPlanes, bps = d->vi->format.bytesPerSample;
    mvx_flowblur_job job;
    memset(&job, 0, sizeof(job));
    void *srcArena = NULL, *dstArena = NULL, *dsrc[3], *ddst[3], *blobB = NULL, *blobF = NULL;
    int height[3] = { 0, 0, 0 };
    for (int p = 0; p < np; p++) height[p] = vs->getFrameHeight(src, p);
    int rc = upload_plane_set(dsrc, &srcArena, src, d->pitch, np, bps, vs);
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->pitch, height, np);
    for (int p = 0; p < np && !rc; p++) { job.clip[p] = dsrc[p]; job.dst[p] = ddst[p]; }
    DevRef ds;
    memset(&ds, 0, sizeof(ds));
    if (!rc) rc = clip_super_to_device(&ds, n, d->super, &d->c.geo, ctx, vs);
    if (!rc && both) rc = clip_blob_to_device(&blobB, n - off, d->mvbw, &d->bw, ctx, vs);
    if (!rc && both) rc = clip_blob_to_device(&blobF, n + off, d->mvfw, &d->fw, ctx, vs);
    for (int p = 0; p < 3; p++) job.super[p] = ds.plane[p];
    job.blob_bw = blobB; job.blob_fw = blobF; /* both NULL: copy of the clip frame */
    if (!rc) rc = mvx_flowblur_frames(d->fb, 1, &job, thread_stream());
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi->format, d->vi->width, d->vi->height, src, core);
        rc = download_plane_set(dst, ddst, d->pitch, np, bps, vs);
    }
    shell_quiesce(rc);
    dev_release(&ds);
    if (blobB) mvx_dev_free(blobB);
    if (blobF) mvx_dev_free(blobF);
    if (srcArena) mvx_dev_free(srcArena);
    if (dstArena) mvx_dev_free(dstArena);
    vs->freeFrame(src);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error("FlowBlur", rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

/* src/MVFlowBlur.c:346-552 */
static void VS_CC blurCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    BlurData *d = (BlurData *)consumer_new(sizeof(*d), "FlowBlur", blurGetFrameUngated, mvx_flowblur_destroy_engine);
    char err[1400] = "";
    mvx_flowblur_args a;
    a.blur = opt_float(in, "blur", 50.0, vs); a.prec = opt_int(in, "prec", vs);
    a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) { d->mvbw = consumer_node(&d->c, in, "mvbw", vs); adata_from_clip(&d->bw, d->mvbw, "FlowBlur", "mvbw", err, sizeof(err), vs); }
    if (!err[0]) { d->mvfw = consumer_node(&d->c, in, "mvfw", vs); adata_from_clip(&d->fw, d->mvfw, "FlowBlur", "mvfw", err, sizeof(err), vs); }
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->vi = vs->getVideoInfo(d->node);
        clip_pitches(d->pitch, d->vi, d->vi->format.bytesPerSample);
        char lerr[MVX_ERRLEN];
        d->c.floatEntry = 1;
        if ((vi_is_float(d->vi) ? mvx_flowblur_create_float : mvx_flowblur_create)(&a, &d->bw, &d->fw, d->c.sup, d->vi->numFrames, d->c.geo.pitch, d->pitch, d->pitch, &d->fb, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        else consumer_check_clip(&d->c, d->vi, vs->getVideoInfo(d->super), 0, err, sizeof(err));
        d->c.engine = d->fb;
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    VSFilterDependency deps[4] = { { d->node, rpStrictSpatial }, { d->super, rpStrictSpatial }, { d->mvbw, rpGeneral }, { d->mvfw, rpGeneral } };
    vs->createVideoFilter(out, "FlowBlur", d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 4, d, core);
}

/* ------------------------------------------------------------------------------------------------ mv.Mask */

typedef struct MaskData { Consumer c; VSNode *node, *vectors; const VSVideoInfo *clipvi; VSVideoInfo vi; mvx_mask *mk; mvx_mask_info info; mvx_analysis_data ad; ptrdiff_t pitch[3]; int kind, bps; } MaskData;
/* MVX_VS_MASK_DEEP=1 (read once, at the entry point): mv.Mask goes through mvx_mask_create_deep, takes clips of 8 to 16 bits and gives a mask of the clip's depth */
static int g_mask_deep;
#define MASK_FORMAT_MSG "Mask: input clip must be GRAY8, YUV420P8, YUV422P8, YUV440P8, or YUV444P8, with constant dimensions."
#define MASK_FORMAT_MSG_DEEP "Mask: input clip must be Gray or YUV (4:2:0, 4:2:2, 4:4:0, 4:4:4) of 8 to 16 bits, with constant dimensions."

static const VSFrame *VS_CC maskGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    MaskData *d = (MaskData *)inst;
    if (reason == arInitial) { /* src/MVMask.c:80-82 */
        vs->requestFrameFilter(n, d->vectors, ctx);
        vs->requestFrameFilter(n, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx); /* the new frame's props; its luma is kind 5's plane 0 */
    mvx_mask_job job;
    memset(&job, 0, sizeof(job));
    void *lumaArena = NULL, *dstArena = NULL, *dluma[3], *ddst[3], *dblob = NULL;
    int rc = 0;
    if (d->kind == 5) rc = upload_plane_set(dluma, &lumaArena, src, d->pitch, 1, d->bps, vs); /* (the clip has the mask's depth: creation) */
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->pitch, d->info.plane_height, 3);
    if (!rc) rc = clip_blob_to_device(&dblob, n, d->vectors, &d->ad, ctx, vs);
    for (int p = 0; p < 3 && !rc; p++) job.dst[p] = ddst[p];
    job.blob = dblob;
    job.clip_luma = d->kind == 5 && !rc ? dluma[0] : NULL;
    if (!rc) rc = mvx_mask_frames(d->mk, 1, &job, thread_stream());
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi.format, d->vi.width, d->vi.height, src, core);
        rc = download_plane_set(dst, ddst, d->pitch, 3, d->bps, vs);
    }
    shell_quiesce(rc);
    if (dblob) mvx_dev_free(dblob);
    if (lumaArena) mvx_dev_free(lumaArena);
    if (dstArena) mvx_dev_free(dstArena);
    vs->freeFrame(src);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error("Mask", rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

/* src/MVMask.c:227-346 */
static void VS_CC maskCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    MaskData *d = (MaskData *)consumer_new(sizeof(*d), "Mask", maskGetFrameUngated, mvx_mask_destroy_engine);
    char err[1400] = "";
    mvx_mask_args a;
    a.ml = opt_float(in, "ml", 100.0, vs); a.gamma = opt_float(in, "gamma", 1.0, vs); a.kind = opt_int(in, "kind", vs); a.time = opt_float(in, "time", 100.0, vs);
    a.ysc = opt_int(in, "ysc", vs); a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    d->kind = a.kind == MVX_UNSET ? 0 : a.kind;
    d->vectors = consumer_node(&d->c, in, "vectors", vs);
    adata_from_clip(&d->ad, d->vectors, "Mask", "vectors", err, sizeof(err), vs);
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->clipvi = vs->getVideoInfo(d->node);
        d->vi = *d->clipvi;
        const VSVideoFormat *f = &d->clipvi->format;
        const mvx_mask_clip mc = { d->clipvi->width, d->clipvi->height, f->bitsPerSample, f->subSamplingW, f->subSamplingH, f->colorFamily == cfGray };
        d->bps = g_mask_deep && f->bitsPerSample > 8 ? 2 : 1;
        clip_pitches(d->pitch, d->clipvi, d->bps); /* of the clip's luma and of the mask's planes alike: the same depth, the clip's subsampling (Gray: none, three full-size planes) */
        char lerr[MVX_ERRLEN];
        if ((g_mask_deep ? mvx_mask_create_deep : mvx_mask_create)(&a, &d->ad, &mc, d->pitch, d->pitch, &d->mk, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        else if (!mvx_vsh_is_constant_video_format(d->clipvi) || f->sampleType != stInteger || (f->colorFamily != cfYUV && f->colorFamily != cfGray))
            snprintf(err, sizeof(err), "%s", g_mask_deep ? MASK_FORMAT_MSG_DEEP : MASK_FORMAT_MSG);
        d->c.engine = d->mk;
    }
    if (!err[0]) { /* three planes with the clip's subsampling, 8-bit (deep: of the clip's depth); Gray -> 4:4:4 (src/MVMask.c:328-329) */
        mvx_mask_get_info(d->mk, &d->info);
        const int obits = mvx_mask_out_bits(d->mk);
        if (!vs->queryVideoFormat(&d->vi.format, cfYUV, stInteger, obits, d->info.subsampling_w, d->info.subsampling_h, core))
            snprintf(err, sizeof(err), "Mask: the host has no %d-bit YUV format for the mask clip.", obits);
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    VSFilterDependency deps[2] = { { d->node, rpStrictSpatial }, { d->vectors, rpStrictSpatial } };
    vs->createVideoFilter(out, "Mask", &d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 2, d, core);
}

/* ------------------------------------------------------------------------------------------------ the Depan family (MVX_VS_DEPAN=1)
 * mv.DepanAnalyse / mv.DepanEstimate write Depan_dx / _dy / _zoom / _rot on copies of the clip's frames, mv.DepanCompensate / mv.DepanStabilise read them from
 * their data clip and warp.  All four sit on the Consumer skeleton (none takes a super clip; DepanEstimate takes no vectors either).  The library's creation
 * functions give the reference's error texts in the reference's order; what only the host can see (a format that is not constant, the sample type, the
 * colour family) reaches them as a bit depth of 0, which draws the reference's format message at its place in that order.  info=1 sets the Depan*_info
 * string with the reference's format from the numbers the library returns and puts text.FrameProps behind the filter (MVDepan.cpp:446-470). */
ENGINE_DESTROY(mvx_depan_analyse) ENGINE_DESTROY(mvx_depan_compensate) ENGINE_DESTROY(mvx_depan_stabilise)

/* a clip's format as the library takes it.  floatSamples NULL: integer clips only (DepanAnalyse, DepanCompensate :2811-2820, DepanStabilise :4025-4034); else DepanEstimate's
 * rule (:1340-1344), a float clip reaching the library as float_samples.  Anything else the reference's format test refuses becomes a bit depth of 0 */
static void depan_clip_of(mvx_depan_clip *c, const VSVideoInfo *vi, int *floatSamples) {
    const VSVideoFormat *f = &vi->format;
    const int isFloat = f->sampleType == stFloat;
    const int known = mvx_vsh_is_constant_video_format(vi) && (f->colorFamily == cfYUV || f->colorFamily == cfGray) && (floatSamples ? 1 : !isFloat);
    c->width = vi->width; c->height = vi->height; c->bits = known ? f->bitsPerSample : 0;
    c->subsampling_w = f->subSamplingW; c->subsampling_h = f->subSamplingH; c->gray = f->colorFamily == cfGray;
    if (floatSamples) *floatSamples = known && isFloat;
}
/* (double)MVX_UNSET where the argument is absent: mvx_depan_stabilise_args */
static double opt_float_unset(const VSMap *in, const char *key, const VSAPI *vs) { return opt_float(in, key, (double)MVX_UNSET, vs); }

/* Depan_dx, _dy, _zoom, _rot of a data frame -> m[0..3] (the library's order); 0 when one is missing */
static int depan_read_motion(float m[4], const VSFrame *f, const VSAPI *vs) {
    static const char *const keys[4] = { "Depan_dx", "Depan_dy", "Depan_zoom", "Depan_rot" };
    const VSMap *props = vs->getFramePropertiesRO(f);
    int ok = 1;
    for (int k = 0; k < 4; k++) { int e = 0; m[k] = (float)vs->mapGetFloat(props, keys[k], 0, &e); if (e) ok = 0; }
    return ok;
}
static void depan_write_motion(VSFrame *dst, const mvx_depan_motion *m, const VSAPI *vs) {
    VSMap *props = vs->getFramePropertiesRW(dst);
    vs->mapSetFloat(props, "Depan_dx", m->dx, maReplace);
    vs->mapSetFloat(props, "Depan_dy", m->dy, maReplace);
    vs->mapSetFloat(props, "Depan_zoom", m->zoom, maReplace);
    vs->mapSetFloat(props, "Depan_rot", m->rot, maReplace);
}
static void depan_set_info(VSFrame *dst, const char *prop, const char *text, const VSAPI *vs) {
    vs->mapSetData(vs->getFramePropertiesRW(dst), prop, text, -1, dtUtf8, maReplace);
}
/* invokeFrameProps, :446-470, and the message its callers put in front.  A host without the text plugin fails creation (the reference hands invoke a NULL plugin) */
static void depan_info_overlay(const char *filter, const char *prop, VSMap *out, VSCore *core, const VSAPI *vs) {
    char msg[700];
    VSPlugin *text = vs->getPluginByID("com.vapoursynth.text", core);
    if (!text) {
        snprintf(msg, sizeof(msg), "%s: failed to invoke text.FrameProps: the host has no plugin com.vapoursynth.text.", filter);
        vs->mapSetError(out, msg);
        return;
    }
    VSNode *node = vs->mapGetNode(out, "clip", 0, NULL);
    VSMap *args = vs->createMap();
    vs->mapSetNode(args, "clip", node, maReplace);
    vs->freeNode(node);
    vs->mapSetData(args, "props", prop, -1, dtUtf8, maReplace);
    VSMap *ret = vs->invoke(text, "FrameProps", args);
    vs->freeMap(args);
    if (vs->mapGetError(ret)) {
        snprintf(msg, sizeof(msg), "%s: failed to invoke text.FrameProps: %s", filter, vs->mapGetError(ret));
        vs->mapSetError(out, msg);
        vs->freeMap(ret);
        return;
    }
    node = vs->mapGetNode(ret, "clip", 0, NULL);
    vs->freeMap(ret);
    vs->mapSetNode(out, "clip", node, maReplace);
    vs->freeNode(node);
}
/* errors of a Depan frame: the library's text as it is (it carries the filter's name where the reference's does) */
static void depan_frame_error(const char *name, int rc, VSFrameContext *ctx, const VSAPI *vs) {
    char msg[MVX_ERRLEN + 64];
    if (rc == MVX_E_NOMEM) { snprintf(msg, sizeof(msg), "%s: out of memory.", name); vs->setFilterError(msg, ctx); }
    else vs->setFilterError(mvx_last_error(), ctx);
}

/* ---- mv.DepanAnalyse, MVDepan.cpp:237-430 / :473-615 */

typedef struct DepanAnalyseData { Consumer c; VSNode *node, *vectors, *mask; const VSVideoInfo *vi; mvx_depan_analyse *da; mvx_analysis_data ad; ptrdiff_t maskPitch[3]; FieldOpt fo; int info; } DepanAnalyseData;

static const VSFrame *VS_CC depanAnalyseGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    DepanAnalyseData *d = (DepanAnalyseData *)inst;
    const int nmv = d->ad.isBackward ? (n > 0 ? n - 1 : 0) : n; /* :287 */
    if (reason == arInitial) { /* :243-247 */
        vs->requestFrameFilter(nmv, d->vectors, ctx);
        vs->requestFrameFilter(n, d->node, ctx);
        if (d->mask) vs->requestFrameFilter(n, d->mask, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    void *dblob = NULL, *maskArena = NULL, *dmask[3] = { NULL, NULL, NULL };
    int rc = clip_blob_to_device(&dblob, nmv, d->vectors, &d->ad, ctx, vs);
    if (rc == MVX_E_ARG) rc = 0; /* an unusable blob: NULL, a frame without a result */
    if (!rc && d->mask) {
        const VSFrame *mf = vs->getFrameFilter(n, d->mask, ctx);
        rc = upload_plane_set(dmask, &maskArena, mf, d->maskPitch, 1, 1, vs);
        vs->freeFrame(mf);
    }
    int missing = 0;
    const int32_t top = d->fo.fields ? frame_top_field(&d->fo, src, n, &missing, vs) : 0;
    mvx_depan_motion m;
    memset(&m, 0, sizeof(m));
    const void *blobs[1] = { dblob }, *masks[1] = { dmask[0] };
    if (!rc) rc = mvx_depan_analyse_frames(d->da, 1, blobs, d->mask ? masks : NULL, d->maskPitch[0], &top, &m, thread_stream());
    shell_quiesce(rc);
    if (dblob) mvx_dev_free(dblob);
    if (maskArena) mvx_dev_free(maskArena);
    if (!rc && missing && m.dx != 0.0f) { /* :371-383: the parity is read for a frame with a result only */
        vs->freeFrame(src);
        vs->setFilterError("DepanAnalyse: _Field property not found in input frame. Therefore, you must pass tff argument.", ctx);
        return NULL;
    }
    if (rc) { vs->freeFrame(src); depan_frame_error("DepanAnalyse", rc, ctx, vs); return NULL; }
    VSFrame *dst = vs->copyFrame(src, core);
    vs->freeFrame(src);
    if (d->info) { /* :405 */
        char info[129];
        snprintf(info, 128, "fn=%d iter=%d error=%.3f dx=%.2f dy=%.2f rot=%.3f zoom=%.5f", n, m.iter, m.error, m.dx, m.dy, m.rot, m.zoom);
        depan_set_info(dst, "DepanAnalyse_info", info, vs);
    }
    depan_write_motion(dst, &m, vs);
    return dst;
}

static void VS_CC depanAnalyseCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    DepanAnalyseData *d = (DepanAnalyseData *)consumer_new(sizeof(*d), "DepanAnalyse", depanAnalyseGetFrameUngated, mvx_depan_analyse_destroy_engine);
    char err[1400] = "", aerr[1400] = "", lerr[MVX_ERRLEN] = "";
    int e = 0;
    mvx_depan_analyse_args a;
    a.zoom = opt_int(in, "zoom", vs); a.rot = opt_int(in, "rot", vs);
    if (a.zoom != MVX_UNSET) a.zoom = !!a.zoom;
    if (a.rot != MVX_UNSET) a.rot = !!a.rot;
    a.pixaspect = opt_float(in, "pixaspect", 1.0, vs); a.error = opt_float(in, "error", 15.0, vs); a.wrong = opt_float(in, "wrong", 10.0, vs); a.zerow = opt_float(in, "zerow", 0.05, vs);
    a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    d->info = !!vs->mapGetInt(in, "info", 0, &e);
    field_opt(&d->fo, in, vs);
    a.fields = d->fo.fields;
    d->node = consumer_node(&d->c, in, "clip", vs);
    d->vi = vs->getVideoInfo(d->node);
    d->vectors = consumer_node(&d->c, in, "vectors", vs);
    d->mask = vs->mapGetNode(in, "mask", 0, &e);
    if (d->mask) d->c.nodes[d->c.nnodes++] = d->mask;
    mvx_depan_clip clip, mclip;
    depan_clip_of(&clip, d->vi, NULL);
    const VSVideoInfo *mvi = d->mask ? vs->getVideoInfo(d->mask) : NULL;
    if (mvi) {
        depan_clip_of(&mclip, mvi, NULL);
        mclip.bits = mvx_vsh_is_constant_video_format(mvi) ? mvi->format.bitsPerSample : 99; /* :558-562: not constant fails as more than 8 bits does */
        clip_pitches(d->maskPitch, mvi, 1);
    }
    /* the reference's order: pixaspect, the clip's format, the lengths, the mask (all from the library but the second), then the vector clip's data (:575), then
     * delta and thscd (the library).  A vector clip without data is tried with a blank one: whatever fails before :575 is reported first */
    const int noData = adata_from_clip(&d->ad, d->vectors, "DepanAnalyse", "vectors", aerr, sizeof(aerr), vs) != 0;
    if (noData) { memset(&d->ad, 0, sizeof(d->ad)); d->ad.nDeltaFrame = 1; }
    if ((float)a.pixaspect > 0.0f && !mvx_vsh_is_constant_video_format(d->vi)) snprintf(err, sizeof(err), "DepanAnalyse: clip must have constant format and dimensions.");
    else if (mvx_depan_analyse_create(&a, &d->ad, &clip, mvi ? &mclip : NULL, d->vi->numFrames, vs->getVideoInfo(d->vectors)->numFrames, mvi ? mvi->numFrames : 0, &d->da, lerr)) {
        static const char *const early[3] = { "DepanAnalyse: pixaspect", "DepanAnalyse: vectors must", "DepanStabilise: mask" };
        int isEarly = 0;
        for (int k = 0; k < 3; k++) if (!strncmp(lerr, early[k], strlen(early[k]))) isEarly = 1;
        snprintf(err, sizeof(err), "%s", noData && !isEarly ? aerr : lerr);
    }
    else if (noData) snprintf(err, sizeof(err), "%s", aerr);
    d->c.engine = d->da;
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    VSFilterDependency deps[3] = { { d->node, rpStrictSpatial }, { d->vectors, rpGeneral }, { d->mask, rpStrictSpatial } };
    vs->createVideoFilter(out, "DepanAnalyse", d->vi, consumerGetFrame, consumerFree, fmParallel, deps, d->mask ? 3 : 2, d, core);
    if (d->info && !vs->mapGetError(out)) depan_info_overlay("DepanAnalyse", "DepanAnalyse_info", out, core, vs);
}

/* ---- mv.DepanEstimate, MVDepan.cpp:956-1243 / :1271-1503.  ONE node where the reference chains three: the spectra the reference hands from stage 1 to stage 2
 * as DepanEstimateFFT / FFT2 properties stay on the device in a small per-instance table of recently used frames, and the stage-2 results it hands to stage 3 as
 * DepanEstimateX / Y / Zoom / Trust properties live in a per-instance table by frame number (16 bytes a frame, each filled once).  Neither kind of property
 * exists here.  The library's results depend on neither batch size nor order, so the output does not depend on the order of the requests.  show=1: the
 * correlate of pair n always runs through mvx_depan_estimate_correlate_show on a device copy of frame n's luma, and the window rows come back. */

#define DE_SPECTRA_SLOTS 8
typedef struct DepanEstimateData {
    Consumer c; VSNode *node; const VSVideoInfo *vi; mvx_depan_estimate *de; mvx_depan_estimate_info ei; ptrdiff_t pitch[3]; int info, show;
    pthread_mutex_t mu;                    /* the two tables, and the device work that fills them */
    mvx_depan_estimate_result *res; unsigned char *have;
    struct { int frame; void *buf; uint64_t stamp; } slot[DE_SPECTRA_SLOTS]; uint64_t clock;
} DepanEstimateData;

static void depan_estimate_destroy_engine(void *e) {
    DepanEstimateData *d = (DepanEstimateData *)e;
    for (int i = 0; i < DE_SPECTRA_SLOTS; i++) if (d->slot[i].buf) mvx_dev_free(d->slot[i].buf);
    free(d->res); free(d->have);
    if (d->de) mvx_depan_estimate_destroy(d->de);
    pthread_mutex_destroy(&d->mu);
}
/* the device spectra of clip frame `frame` (mu held); `keep`: a frame whose slot must survive */
static int depan_estimate_spectra_of(DepanEstimateData *d, int frame, int keep, void **out, VSFrameContext *ctx, const VSAPI *vs) {
    int lru = -1;
    for (int i = 0; i < DE_SPECTRA_SLOTS; i++) {
        if (d->slot[i].buf && d->slot[i].frame == frame) { d->slot[i].stamp = ++d->clock; *out = d->slot[i].buf; return 0; }
        if (d->slot[i].buf && d->slot[i].frame == keep) continue;
        if (lru < 0 || !d->slot[i].buf || (d->slot[lru].buf && d->slot[i].stamp < d->slot[lru].stamp)) lru = i;
    }
    if (!d->slot[lru].buf) d->slot[lru].buf = shell_alloc((size_t)d->ei.windows * (size_t)d->ei.spectrum_bytes);
    if (!d->slot[lru].buf) return MVX_E_NOMEM;
    d->slot[lru].frame = -1;
    const VSFrame *f = vs->getFrameFilter(frame, d->node, ctx);
    void *arena = NULL, *plane[3];
    int rc = upload_plane_set(plane, &arena, f, d->pitch, 1, d->vi->format.bytesPerSample, vs);
    vs->freeFrame(f);
    const void *planes[1] = { plane[0] };
    void *spectra[1] = { d->slot[lru].buf };
    if (!rc) rc = mvx_depan_estimate_spectra(d->de, 1, planes, d->pitch[0], spectra, thread_stream());
    if (!rc) rc = mvx_stream_sync(thread_stream()); /* another thread's stream reads them next */
    shell_quiesce(rc);
    if (arena) mvx_dev_free(arena);
    if (rc) return rc;
    d->slot[lru].frame = frame; d->slot[lru].stamp = ++d->clock;
    *out = d->slot[lru].buf;
    return 0;
}

static const VSFrame *VS_CC depanEstimateGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    DepanEstimateData *d = (DepanEstimateData *)inst;
    const int last = d->vi->numFrames - 1;
    const int lo = n - 2 > 0 ? n - 2 : 0, hi = n + 1 < last ? n + 1 : last;
    if (reason == arInitial) { /* stage 3 reads the results of n - 1 .. n + 1 (:1160-1162), stage 2 of a frame reads the frame before it too (:1005-1006) */
        for (int k = lo; k <= hi; k++) vs->requestFrameFilter(k, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    VSFrame *dst = vs->copyFrame(src, core);
    vs->freeFrame(src);
    const int want[3] = { n > 0 ? n - 1 : 0, n, n < last ? n + 1 : last };
    const int bps = d->vi->format.bytesPerSample;
    int rc = 0;
    pthread_mutex_lock(&d->mu);
    for (int k = 0; k < 3 && !rc; k++) {
        const int r = want[k], paint = d->show && r == n && k == 1;
        if (d->have[r] && !paint) continue;
        const int p = r > 0 ? r - 1 : 0; /* frame 0 is its own predecessor, :1009 */
        void *sprev = NULL, *scur = NULL;
        rc = depan_estimate_spectra_of(d, p, r, &sprev, ctx, vs);
        if (!rc) rc = depan_estimate_spectra_of(d, r, p, &scur, ctx, vs);
        if (rc) break;
        const VSFrame *fr = vs->getFrameFilter(r, d->node, ctx);
        int e = 0;
        const int field = !!vs->mapGetInt(vs->getFramePropertiesRO(fr), "_Field", 0, &e);
        const int32_t top = e ? MVX_UNSET : field, num = r;
        const void *pp[1] = { sprev }, *cp[1] = { scur };
        mvx_depan_estimate_result res;
        if (!paint) rc = mvx_depan_estimate_correlate(d->de, 1, pp, cp, &top, &num, &res, NULL, thread_stream());
        else {
            void *arena = NULL, *plane[3];
            rc = upload_plane_set(plane, &arena, fr, d->pitch, 1, bps, vs);
            void *planes[1] = { plane[0] };
            if (!rc) rc = mvx_depan_estimate_correlate_show(d->de, 1, pp, cp, &top, &num, &res, NULL, planes, d->pitch[0], thread_stream());
            if (!rc) rc = timed_download(vs->getWritePtr(dst, 0) + (size_t)d->ei.wtop * vs->getStride(dst, 0), vs->getStride(dst, 0),
                                         (char *)plane[0] + (size_t)d->ei.wtop * d->pitch[0], d->pitch[0], (size_t)d->vi->width * bps, (size_t)d->ei.winy);
            if (!rc) rc = mvx_stream_sync(thread_stream());
            shell_quiesce(rc);
            if (arena) mvx_dev_free(arena);
        }
        vs->freeFrame(fr);
        if (!rc) { d->res[r] = res; d->have[r] = 1; }
    }
    mvx_depan_estimate_result tri[3];
    if (!rc) for (int k = 0; k < 3; k++) tri[k] = d->res[want[k]];
    pthread_mutex_unlock(&d->mu);
    shell_quiesce(rc);
    mvx_depan_motion m;
    if (!rc) rc = mvx_depan_estimate_finish(d->de, n, tri, &m);
    if (rc) { vs->freeFrame(dst); depan_frame_error("DepanEstimate", rc, ctx, vs); return NULL; }
    depan_write_motion(dst, &m, vs);
    if (d->info) { /* :1233 */
        char info[129];
        snprintf(info, 128, "fn=%d dx=%.2f dy=%.2f zoom=%.5f trust=%.2f", n, m.dx, m.dy, m.zoom, tri[1].trust);
        depan_set_info(dst, "DepanEstimate_info", info, vs);
    }
    return dst;
}

static void VS_CC depanEstimateCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    DepanEstimateData *d = (DepanEstimateData *)consumer_new(sizeof(*d), "DepanEstimate", depanEstimateGetFrameUngated, depan_estimate_destroy_engine);
    pthread_mutex_init(&d->mu, NULL);
    d->c.engine = d;
    char lerr[MVX_ERRLEN] = "";
    int e = 0, floatSamples = 0;
    mvx_depan_estimate_args a;
    a.trust = opt_float(in, "trust", 4.0, vs); a.zoommax = opt_float(in, "zoommax", 1.0, vs); a.stab = opt_float(in, "stab", 1.0, vs); a.pixaspect = opt_float(in, "pixaspect", 1.0, vs);
    a.winx = opt_int(in, "winx", vs); a.winy = opt_int(in, "winy", vs); a.wleft = opt_int(in, "wleft", vs); a.wtop = opt_int(in, "wtop", vs);
    a.dxmax = opt_int(in, "dxmax", vs); a.dymax = opt_int(in, "dymax", vs);
    FieldOpt fo;
    field_opt(&fo, in, vs);
    a.fields = fo.fields; a.tff = fo.tffExists ? fo.tff : MVX_UNSET;
    d->info = !!vs->mapGetInt(in, "info", 0, &e);
    d->show = !!vs->mapGetInt(in, "show", 0, &e);
    d->node = consumer_node(&d->c, in, "clip", vs);
    d->vi = vs->getVideoInfo(d->node);
    mvx_depan_clip clip;
    depan_clip_of(&clip, d->vi, &floatSamples);
    a.float_samples = floatSamples;
    if (mvx_depan_estimate_create(&a, &clip, d->vi->numFrames, &d->de, lerr)) { consumer_fail(&d->c, lerr, out, vs); return; }
    mvx_depan_estimate_get_info(d->de, &d->ei);
    clip_pitches(d->pitch, d->vi, d->vi->format.bytesPerSample);
    d->res = (mvx_depan_estimate_result *)calloc((size_t)d->vi->numFrames, sizeof(*d->res));
    d->have = (unsigned char *)calloc((size_t)d->vi->numFrames, 1);
    if (!d->res || !d->have) { consumer_fail(&d->c, "DepanEstimate: out of memory.", out, vs); return; }
    VSFilterDependency deps[1] = { { d->node, rpGeneral } };
    vs->createVideoFilter(out, "DepanEstimate", d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 1, d, core);
    if (d->info && !vs->mapGetError(out)) depan_info_overlay("DepanEstimate", "DepanEstimate_info", out, core, vs);
}

/* ---- what mv.DepanCompensate (dc, ci) and mv.DepanStabilise (ds) share: the instance, the opening and the end of creation, the tail of a frame */
typedef struct DepanWarpData { Consumer c; VSNode *node, *data; const VSVideoInfo *vi; ptrdiff_t pitch[3]; int height[3], info, flt /* a float clip: the float entries */; mvx_depan_compensate *dc; mvx_depan_compensate_info ci; mvx_depan_stabilise *ds; } DepanWarpData;

/* the instance with its clip and data nodes, the clip's format as the library takes it, and the pitches and heights of the device planes */
static DepanWarpData *depan_warp_open(const char *name, VSFilterGetFrame body, void (*destroy)(void *), const VSMap *in, mvx_depan_clip *clip, const VSAPI *vs) {
    DepanWarpData *d = (DepanWarpData *)consumer_new(sizeof(*d), name, body, destroy);
    int e = 0;
    d->info = !!vs->mapGetInt(in, "info", 0, &e);
    d->node = consumer_node(&d->c, in, "clip", vs);
    d->vi = vs->getVideoInfo(d->node);
    d->data = consumer_node(&d->c, in, "data", vs);
    depan_clip_of(clip, d->vi, NULL);
    /* MVX_VS_FLOAT=1: a float clip of a constant Gray or YUV format goes to the library's float entry with its 32 bits; every other float clip stays a bit depth of 0 */
    d->flt = vi_is_float(d->vi) && mvx_vsh_is_constant_video_format(d->vi) && (d->vi->format.colorFamily == cfYUV || d->vi->format.colorFamily == cfGray);
    if (d->flt) clip->bits = 32;
    clip_pitches(d->pitch, d->vi, d->vi->format.bytesPerSample > 0 ? d->vi->format.bytesPerSample : 1);
    for (int p = 0; p < 3; p++) d->height[p] = p ? d->vi->height >> d->vi->format.subSamplingH : d->vi->height;
    return d;
}
/* after the library's creation: the engine handed to the skeleton, the filter, and with info=1 text.FrameProps behind it */
static void depan_warp_register(DepanWarpData *d, const char *name, const char *prop, void *engine, VSMap *out, VSCore *core, const VSAPI *vs) {
    d->c.engine = engine;
    VSFilterDependency deps[2] = { { d->node, rpGeneral }, { d->data, rpGeneral } };
    vs->createVideoFilter(out, name, d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 2, d, core);
    if (d->info && !vs->mapGetError(out)) depan_info_overlay(name, prop, out, core, vs);
}
/* rc: what the uploads of the job's sources gave.  Allocates the destination planes into jobDst (the job's dst member), launches the one job, downloads into a new
 * frame with src's properties, and frees the arenas and src.  NULL, with the filter error set, when any step failed */
static VSFrame *depan_warp_finish(DepanWarpData *d, const char *name, int rc, const void *job, void *jobDst[3], void *const *arena, int narena, const VSFrame *src,
        VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    const int np = d->vi->format.numPlanes, bps = d->vi->format.bytesPerSample;
    void *dstArena = NULL, *ddst[3];
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->pitch, d->height, np);
    for (int p = 0; p < np && !rc; p++) jobDst[p] = ddst[p];
    if (!rc) rc = d->ds ? mvx_depan_stabilise_frames(d->ds, 1, (const mvx_depan_stabilise_job *)job, thread_stream())
                        : mvx_depan_compensate_frames(d->dc, 1, (const mvx_depan_compensate_job *)job, thread_stream());
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->vi->format, d->vi->width, d->vi->height, src, core);
        rc = download_plane_set(dst, ddst, d->pitch, np, bps, vs);
    }
    shell_quiesce(rc);
    for (int k = 0; k < narena; k++) if (arena[k]) mvx_dev_free(arena[k]);
    if (dstArena) mvx_dev_free(dstArena);
    vs->freeFrame(src);
    if (rc) { if (dst) vs->freeFrame(dst); depan_frame_error(name, rc, ctx, vs); return NULL; }
    return dst;
}

/* ---- mv.DepanCompensate, MVDepan.cpp:2588-2735 / :2750-2881 */

static const VSFrame *VS_CC depanCompGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    DepanWarpData *d = (DepanWarpData *)inst;
    int nsrc = n, start = n, end = n;
    const int warp = mvx_depan_compensate_map(d->dc, n, &nsrc, &start, &end);
    if (reason == arInitial) { /* :2594-2609 */
        if (warp) {
            vs->requestFrameFilter(nsrc, d->node, ctx);
            for (int k = start + 1; k <= end; k++) vs->requestFrameFilter(k, d->data, ctx);
        }
        vs->requestFrameFilter(n, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    if (!warp) return vs->getFrameFilter(n, d->node, ctx); /* :2613-2614 */
    float motions[4 * 24], trsum[6], motion[4];
    int count = 0;
    for (int k = start + 1; k <= end && count < 24; k++, count++) {
        const VSFrame *df = vs->getFrameFilter(k, d->data, ctx);
        const int ok = depan_read_motion(motions + 4 * count, df, vs);
        vs->freeFrame(df);
        if (!ok) { vs->setFilterError("DepanCompensate: required frame properties not found in data clip. Did data clip really come from DepanAnalyse or DepanEstimate?", ctx); return NULL; }
    }
    const VSFrame *cur = vs->getFrameFilter(n, d->node, ctx);
    int e = 0;
    const int field = !!vs->mapGetInt(vs->getFramePropertiesRO(cur), "_Field", 0, &e);
    vs->freeFrame(cur);
    char lerr[MVX_ERRLEN] = "";
    if (mvx_depan_motion_to_transform(d->dc, count, motions, n, e ? MVX_UNSET : field, trsum, motion, lerr)) { vs->setFilterError(lerr, ctx); return NULL; }
    const VSFrame *src = vs->getFrameFilter(nsrc, d->node, ctx);
    const int np = d->vi->format.numPlanes;
    mvx_depan_compensate_job job;
    memset(&job, 0, sizeof(job));
    void *srcArena = NULL, *dsrc[3];
    const int rc = upload_plane_set(dsrc, &srcArena, src, d->pitch, np, d->vi->format.bytesPerSample, vs);
    for (int p = 0; p < np && !rc; p++) job.src[p] = dsrc[p];
    memcpy(job.tr, trsum, sizeof(job.tr));
    VSFrame *dst = depan_warp_finish(d, "DepanCompensate", rc, &job, job.dst, &srcArena, 1, src, ctx, core, vs);
    if (dst && d->info) { /* :2724 */
        char info[129];
        snprintf(info, 128, "offset=%.2f, %d to %d, dx=%.2f, dy=%.2f, rot=%.3f zoom=%.5f", d->ci.offset, nsrc, n, motion[0], motion[1], motion[3], motion[2]);
        depan_set_info(dst, "DepanCompensate_info", info, vs);
    }
    return dst;
}

static void VS_CC depanCompCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    mvx_depan_clip clip;
    DepanWarpData *d = depan_warp_open("DepanCompensate", depanCompGetFrameUngated, mvx_depan_compensate_destroy_engine, in, &clip, vs);
    char lerr[MVX_ERRLEN] = "";
    mvx_depan_compensate_args a;
    a.offset = opt_float(in, "offset", 0.0, vs); a.subpixel = opt_int(in, "subpixel", vs); a.pixaspect = opt_float(in, "pixaspect", 1.0, vs);
    a.matchfields = opt_int(in, "matchfields", vs); a.mirror = opt_int(in, "mirror", vs); a.blur = opt_int(in, "blur", vs);
    FieldOpt fo;
    field_opt(&fo, in, vs);
    a.fields = fo.fields; a.tff = fo.tffExists ? fo.tff : MVX_UNSET;
    if ((d->flt ? mvx_depan_compensate_create_float : mvx_depan_compensate_create)(&a, &clip, d->vi->numFrames, vs->getVideoInfo(d->data)->numFrames, d->pitch, d->pitch, &d->dc, lerr)) { consumer_fail(&d->c, lerr, out, vs); return; }
    mvx_depan_compensate_get_info(d->dc, &d->ci);
    depan_warp_register(d, "DepanCompensate", "DepanCompensate_info", d->dc, out, core, vs);
}

/* ---- mv.DepanStabilise, MVDepan.cpp:3562-3885 / :3909-4208 */

static const VSFrame *VS_CC depanStabGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    DepanWarpData *d = (DepanWarpData *)inst;
    int df = n, dl = n, cf = n, cl = n;
    int rc = mvx_depan_stabilise_window(d->ds, n, &df, &dl, &cf, &cl);
    if (rc) { if (reason == arInitial || reason == arAllFramesReady) depan_frame_error("DepanStabilise", rc, ctx, vs); return NULL; }
    if (reason == arInitial) { /* :3571-3591, :3720-3763, and the data frames of the library's divergence 5 */
        for (int k = df; k <= dl; k++) vs->requestFrameFilter(k, d->data, ctx);
        for (int k = cf; k <= cl; k++) vs->requestFrameFilter(k, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    float *motions = (float *)malloc(sizeof(float) * 4 * (size_t)(dl - df + 1));
    if (!motions) { vs->setFilterError("DepanStabilise: out of memory.", ctx); return NULL; }
    for (int k = df; k <= dl; k++) {
        const VSFrame *f = vs->getFrameFilter(k, d->data, ctx);
        const int ok = depan_read_motion(motions + 4 * (size_t)(k - df), f, vs);
        vs->freeFrame(f);
        if (!ok && k != 0) { /* (data frame 0 is never read, :4075-4078) */
            free(motions);
            vs->setFilterError("DepanStabilise: required frame properties not found in data clip.", ctx); /* :3343 */
            return NULL;
        }
    }
    char lerr[MVX_ERRLEN] = "";
    mvx_depan_stabilise_job job;
    memset(&job, 0, sizeof(job));
    rc = mvx_depan_stabilise_plan(d->ds, n, motions, &job.plan, lerr);
    free(motions);
    if (rc) { vs->setFilterError(lerr, ctx); return NULL; }
    const int np = d->vi->format.numPlanes, bps = d->vi->format.bytesPerSample;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    void *arena[3] = { NULL, NULL, NULL }, *dcur[3], *dprev[3], *dnext[3];
    rc = upload_plane_set(dcur, &arena[0], src, d->pitch, np, bps, vs);
    if (!rc && job.plan.prev.used) {
        const VSFrame *f = vs->getFrameFilter(job.plan.prev.frame, d->node, ctx);
        rc = f ? upload_plane_set(dprev, &arena[1], f, d->pitch, np, bps, vs) : MVX_E_ARG;
        vs->freeFrame(f);
    }
    if (!rc && job.plan.next.used) {
        const VSFrame *f = vs->getFrameFilter(job.plan.next.frame, d->node, ctx);
        rc = f ? upload_plane_set(dnext, &arena[2], f, d->pitch, np, bps, vs) : MVX_E_ARG;
        vs->freeFrame(f);
    }
    for (int p = 0; p < np && !rc; p++) {
        job.cur[p] = dcur[p];
        if (job.plan.prev.used) job.prev[p] = dprev[p];
        if (job.plan.next.used) job.next[p] = dnext[p];
    }
    VSFrame *dst = depan_warp_finish(d, "DepanStabilise", rc, &job, job.dst, arena, 3, src, ctx, core, vs);
    if (dst && d->info) { /* :3554 */
        char info[129];
        snprintf(info, 128, "frame=%d %s=%d dx=%.2f dy=%.2f rot=%.3f zoom=%.5f", n, job.plan.base ? "BASE!" : "base ", job.plan.nbase, job.plan.motion[0], job.plan.motion[1],
                 job.plan.motion[3], job.plan.motion[2]);
        depan_set_info(dst, "DepanStabilise_info", info, vs);
    }
    return dst;
}

static void VS_CC depanStabCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    mvx_depan_clip clip;
    DepanWarpData *d = depan_warp_open("DepanStabilise", depanStabGetFrameUngated, mvx_depan_stabilise_destroy_engine, in, &clip, vs);
    char lerr[MVX_ERRLEN] = "";
    mvx_depan_stabilise_args a;
    a.cutoff = opt_float_unset(in, "cutoff", vs); a.damping = opt_float_unset(in, "damping", vs); a.initzoom = opt_float_unset(in, "initzoom", vs);
    a.dxmax = opt_float_unset(in, "dxmax", vs); a.dymax = opt_float_unset(in, "dymax", vs); a.zoommax = opt_float_unset(in, "zoommax", vs); a.rotmax = opt_float_unset(in, "rotmax", vs);
    a.pixaspect = opt_float_unset(in, "pixaspect", vs); a.tzoom = opt_float_unset(in, "tzoom", vs);
    a.addzoom = opt_int(in, "addzoom", vs); a.prev = opt_int(in, "prev", vs); a.next = opt_int(in, "next", vs); a.mirror = opt_int(in, "mirror", vs); a.blur = opt_int(in, "blur", vs);
    a.subpixel = opt_int(in, "subpixel", vs); a.fitlast = opt_int(in, "fitlast", vs); a.method = opt_int(in, "method", vs); a.fields = opt_int(in, "fields", vs);
    if ((d->flt ? mvx_depan_stabilise_create_float : mvx_depan_stabilise_create)(&a, &clip, d->vi->numFrames, vs->getVideoInfo(d->data)->numFrames, d->vi->fpsNum, d->vi->fpsDen, d->pitch, d->pitch, &d->ds, lerr)) { consumer_fail(&d->c, lerr, out, vs); return; }
    depan_warp_register(d, "DepanStabilise", "DepanStabilise_info", d->ds, out, core, vs);
}

/* ------------------------------------------------------------------------------------------------ the temporal-radius filters (MVX_VS_MULTI=1)
 * mv.AnalyseN / mv.RecalculateN / mv.DegrainN / mv.CompensateN / mv.MultiField over the multi blob of include/mvtools_amd.h.  A MULTI VECTOR CLIP is, like mv.Analyse's
 * vector clip, copyFrame(super[n]) with binary properties -- but its own:
 *     MVTools_multi_MVAnalysisData  the 84 bytes of field 0 (backward, delta 1)
 *     MVTools_multi_radius          int
 *     MVTools_multi_stride          int: bytes from one field to the next (a field's size rounded up to 256)
 *     MVTools_multi_vectors         2 * radius * stride bytes; field r at r * stride, every pad byte 0
 * It carries neither MVTools_MVAnalysisData nor MVTools_vectors, so a single-field filter refuses it at creation with its own "Property ... not found" message;
 * mv.MultiField turns one field into an ordinary vector clip.  The property is uploaded per request: handing the blob from mv.AnalyseN's windows to this plugin's consumers on the device was built and
 * measured, and gained nothing beyond the spread of the rates (profiles/multi_lookahead_bench.txt), so it is not here. */
#define PROP_MULTI_ADATA "MVTools_multi_MVAnalysisData"
#define PROP_MULTI_RADIUS "MVTools_multi_radius"
#define PROP_MULTI_STRIDE "MVTools_multi_stride"
#define PROP_MULTI_VECTORS "MVTools_multi_vectors"
#define MULTI_MAX_FIELDS (2 * MVX_DEGRAIN_N_MAX_RADIUS)

typedef struct MultiInfo { mvx_analysis_data ad0; int radius; int64_t stride; } MultiInfo;

/* the analysis data of field r, from field 0's: the one place that knows the order of the fields (mvbw1, mvfw1, mvbw2, mvfw2, ...) */
static void multi_field_data(mvx_analysis_data *out, const mvx_analysis_data *ad0, int r) {
    *out = *ad0;
    out->isBackward = r % 2 == 0;
    out->nDeltaFrame = r / 2 + 1;
    out->nMotionFlags = (ad0->nMotionFlags & ~2) | (out->isBackward ? 2 : 0); /* MOTION_IS_BACKWARD, src/MVAnalyse.c:489 */
}
/* frame n + multi_offset(r) is the reference of field r */
static int multi_offset(int r) { return mvx_win_field_offset(r); }

static int multi_from_clip(MultiInfo *mi, VSNode *clip, const char *filter, const char *name, char *error, size_t esz, const VSAPI *vs) {
    char msg[1024];
    const VSFrame *f0 = vs->getFrame(0, clip, msg, sizeof(msg));
    if (!f0) { snprintf(error, esz, "%s: Failed to retrieve first frame from %s. Error message: %s", filter, name, msg); return -1; }
    const VSMap *props = vs->getFramePropertiesRO(f0);
    int err = 0, e1 = 0, e2 = 0, rc = 0;
    const char *data = vs->mapGetData(props, PROP_MULTI_ADATA, 0, &err);
    if (err) { snprintf(error, esz, "%s: Property '%s' not found in first frame of %s.", filter, PROP_MULTI_ADATA, name); rc = -1; }
    else {
        const int size = vs->mapGetDataSize(props, PROP_MULTI_ADATA, 0, NULL);
        mi->radius = vs->mapGetIntSaturated(props, PROP_MULTI_RADIUS, 0, &e1);
        mi->stride = vs->mapGetInt(props, PROP_MULTI_STRIDE, 0, &e2);
        if (size != (int)sizeof(mi->ad0)) { snprintf(error, esz, "%s: Property '%s' in first frame of %s has wrong size (%d instead of %d).", filter, PROP_MULTI_ADATA, name, size, (int)sizeof(mi->ad0)); rc = -1; }
        else if (e1 || e2 || mi->radius < 1 || mi->radius > MVX_DEGRAIN_N_MAX_RADIUS || mi->stride < 256 || mi->stride % 256 || mi->stride > (1 << 30)) {
            snprintf(error, esz, "%s: the multi vector clip properties in first frame of %s appear to be wrong.", filter, name); rc = -1;
        } else memcpy(&mi->ad0, data, sizeof(mi->ad0));
    }
    vs->freeFrame(f0);
    return rc;
}

/* the first `nfields` fields of MVTools_multi_vectors of a frame, each validated like a MVTools_vectors property (blob_check: its stated size, here also against the
 * stride, and plane headers that tile it exactly) -> host pointer, or NULL */
static const char *multi_fields_checked(const MultiInfo *mi, int nfields, const VSFrame *vf, const VSAPI *vs) {
    int e = 0;
    const VSMap *props = vs->getFramePropertiesRO(vf);
    const char *blob = vs->mapGetData(props, PROP_MULTI_VECTORS, 0, &e);
    if (e) return NULL;
    const int64_t n = vs->mapGetDataSize(props, PROP_MULTI_VECTORS, 0, NULL);
    if (n != 2 * (int64_t)mi->radius * mi->stride || nfields > 2 * mi->radius) return NULL;
    for (int r = 0; r < nfields; r++) {
        const char *f = blob + (size_t)r * (size_t)mi->stride;
        int stated = 0;
        memcpy(&stated, f, sizeof(stated));
        if (stated < 8 || ((int64_t)stated + 255) / 256 * 256 != mi->stride || blob_check(f, stated, &mi->ad0)) return NULL;
    }
    return blob;
}
static int multi_to_device(void **dblob, const MultiInfo *mi, int nfields, const VSFrame *vf, const VSAPI *vs) {
    *dblob = NULL;
    const char *blob = multi_fields_checked(mi, nfields, vf, vs);
    if (!blob) return MVX_E_ARG;
    const size_t n = (size_t)nfields * (size_t)mi->stride;
    *dblob = shell_alloc(n);
    if (!*dblob) return MVX_E_NOMEM;
    return timed_upload(*dblob, (ptrdiff_t)n, blob, (ptrdiff_t)n, n, 1) ? MVX_E_DEVICE : 0; /* complete on return: the prop memory goes away with the frame */
}
/* a finished multi blob on the device -> the properties of a frame.  Field by field: the device never writes the pad bytes, the property's are 0 */
static int multi_set_props(VSFrame *dst, const void *dblob, const MultiInfo *mi, size_t fieldSize, const VSAPI *vs) {
    const size_t n = 2 * (size_t)mi->radius * (size_t)mi->stride;
    char *host = (char *)calloc(1, n);
    if (!host) return MVX_E_NOMEM;
    int rc = timed_download(host, (ptrdiff_t)mi->stride, dblob, (ptrdiff_t)mi->stride, fieldSize, 2 * (size_t)mi->radius);
    if (!rc) rc = mvx_stream_sync(thread_stream());
    if (!rc) {
        VSMap *props = vs->getFramePropertiesRW(dst);
        vs->mapSetData(props, PROP_MULTI_ADATA, (const char *)&mi->ad0, sizeof(mi->ad0), dtBinary, maReplace);
        vs->mapSetInt(props, PROP_MULTI_RADIUS, mi->radius, maReplace);
        vs->mapSetInt(props, PROP_MULTI_STRIDE, mi->stride, maReplace);
        vs->mapSetData(props, PROP_MULTI_VECTORS, host, (int)n, dtBinary, maReplace);
    }
    free(host);
    return rc;
}
/* the super frames n + multi_offset(r), r < nfields, that lie inside the clip: requested (arInitial) ... */
static void multi_request_refs(int n, int nfields, int numFrames, VSNode *super, VSFrameContext *ctx, const VSAPI *vs) {
    for (int r = 0; r < nfields; r++) {
        const int m = n + multi_offset(r);
        if (m >= 0 && m < numFrames) vs->requestFrameFilter(m, super, ctx);
    }
}
/* ... and brought to the device as the HOST table the *_n jobs take (an entry outside the clip stays NULL) */
static int multi_refs_to_device(DevRef *refs, const void *table[][3], int n, int nfields, int numFrames, VSNode *super, const SuperGeo *g, VSFrameContext *ctx, const VSAPI *vs) {
    int rc = 0;
    for (int r = 0; r < nfields && !rc; r++) {
        const int m = n + multi_offset(r);
        if (m < 0 || m >= numFrames) continue;
        rc = clip_super_to_device(&refs[r], m, super, g, ctx, vs);
        for (int p = 0; p < 3 && !rc; p++) table[r][p] = refs[r].plane[p];
    }
    return rc;
}

ENGINE_DESTROY(mvx_analyse_n) ENGINE_DESTROY(mvx_recalculate_n) ENGINE_DESTROY(mvx_degrain_n) ENGINE_DESTROY(mvx_compensate_n)

/* ---- mv.AnalyseN(super, radius, ...).  Under mv.Analyse's conditions it computes its clip in look-ahead windows (the engine above): ONE mvx_analyse_n_frames call per
 * window of MVX_VS_MULTI_LOOKAHEAD frames (unset: mvx_win_default_length; 0: off), whose multi blobs stay on the device until the slot is recycled; a request
 * downloads its frame's fields from there.  Else, and for a request that finds no slot, one call per frame (no combining queue). */
typedef struct AnalyseNData { Consumer c; VSNode *super; const VSVideoInfo *vi; mvx_analyse_n *an; MultiInfo mi; size_t fieldSize; FieldOpt fo; LookAhead la; } AnalyseNData;

static const VSFrame *VS_CC analyseNGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    AnalyseNData *d = (AnalyseNData *)inst;
    const int nf = 2 * d->mi.radius;
    if (reason == arInitial) {
        vs->requestFrameFilter(n, d->super, ctx);
        multi_request_refs(n, nf, d->vi->numFrames, d->super, ctx, vs);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->super, ctx);
    int32_t shift[MULTI_MAX_FIELDS];
    memset(shift, 0, sizeof(shift));
    if (d->fo.fields) { /* src/MVAnalyse.c:135-179, per field */
        int missing = 0;
        const int srcTop = frame_top_field(&d->fo, src, n, &missing, vs);
        for (int r = 0; r < nf; r++) {
            const int m = n + multi_offset(r);
            if (m < 0 || m >= d->vi->numFrames) continue;
            const VSFrame *ref = vs->getFrameFilter(m, d->super, ctx);
            const int refTop = frame_top_field(&d->fo, ref, m, &missing, vs);
            vs->freeFrame(ref);
            if (d->mi.ad0.nPel > 1 && (r / 2 + 1) % 2) shift[r] = field_shift_of(srcTop, refTop, d->mi.ad0.nPel);
        }
        if (missing) {
            vs->setFilterError("AnalyseN: _Field property not found in input frame. Therefore, you must pass tff argument.", ctx);
            vs->freeFrame(src);
            return NULL;
        }
    }
    DevRef ds, refs[MULTI_MAX_FIELDS];
    const void *table[MULTI_MAX_FIELDS][3];
    memset(refs, 0, sizeof(refs)); memset(table, 0, sizeof(table));
    int rc = super_to_device(&ds, src, &d->c.geo, vs);
    if (!rc) rc = multi_refs_to_device(refs, table, n, nf, d->vi->numFrames, d->super, &d->c.geo, ctx, vs);
    void *dblob = rc ? NULL : shell_alloc(2 * (size_t)d->mi.radius * (size_t)d->mi.stride);
    if (!rc && !dblob) rc = MVX_E_NOMEM;
    VSFrame *dst = NULL;
    if (!rc) {
        mvx_analyse_n_job job;
        memset(&job, 0, sizeof(job));
        for (int p = 0; p < 3; p++) job.src[p] = ds.plane[p];
        job.refs = table; job.blob = dblob; job.field_shift = shift;
        rc = mvx_analyse_n_frames(d->an, 1, &job, thread_stream());
        if (!rc) { dst = vs->copyFrame(src, core); rc = multi_set_props(dst, dblob, &d->mi, d->fieldSize, vs); }
    }
    shell_quiesce(rc);
    dev_release(&ds);
    for (int r = 0; r < nf; r++) dev_release(&refs[r]);
    if (dblob) mvx_dev_free(dblob);
    vs->freeFrame(src);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error(d->c.name, rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

/* mv.AnalyseN's launch: one job per frame of the window, its 2 * radius references from a HOST table of count x 2 * radius entries (outside the clip: NULL) */
static int analyse_n_enqueue(void *owner, const LaLaunch *l) {
    AnalyseNData *d = (AnalyseNData *)owner;
    const int nf = 2 * d->mi.radius;
    const size_t cells = (size_t)l->count * (size_t)nf;
    const void *(*table)[3] = (const void *(*)[3])calloc(cells, sizeof(*table));
    int32_t *shift = (int32_t *)calloc(cells, sizeof(int32_t));
    mvx_analyse_n_job *jobs = (mvx_analyse_n_job *)calloc((size_t)l->count, sizeof(mvx_analyse_n_job));
    int rc = (!table || !shift || !jobs) ? MVX_E_NOMEM : 0;
    for (int i = 0; i < l->count && !rc; i++) {
        const int n = l->first + i, is = n - l->lo;
        for (int r = 0; r < nf; r++) {
            const int ir = mvx_win_field_input(n, r, l->lo, l->hi);
            if (ir < 0) continue;
            for (int p = 0; p < 3; p++) table[(size_t)i * nf + r][p] = l->pins[ir]->plane[p];
            if (d->fo.fields && d->mi.ad0.nPel > 1 && (r / 2 + 1) % 2) shift[(size_t)i * nf + r] = field_shift_of(l->top[is], l->top[ir], d->mi.ad0.nPel); /* src/MVAnalyse.c:135-179, per field */
        }
        for (int p = 0; p < 3; p++) jobs[i].src[p] = l->pins[is]->plane[p];
        jobs[i].refs = table + (size_t)i * nf; jobs[i].field_shift = shift + (size_t)i * nf;
        jobs[i].blob = (char *)l->dblobs + d->la.frameBytes * (size_t)i;
    }
    if (!rc) rc = mvx_analyse_n_frames(d->an, l->count, jobs, l->stream); /* (the host arrays are read before it returns) */
    free(table); free(shift); free(jobs);
    if (rc) return rc; /* (the AnalyseN line counts windows that were launched) */
    pthread_mutex_lock(&g_lock);
    g_statn_windows++; g_statn_frames += l->count; g_statn_chains += (long)l->count * nf; if (l->count > g_statn_largest) g_statn_largest = l->count;
    pthread_mutex_unlock(&g_lock);
    return 0;
}

/* the node's getFrame when the instance has windows.  A request in a window is ungated, like mv.Analyse's: it waits for GPU work or for a thread that is already running.
 * One that finds no slot, or comes after the instance ran out of device memory, is the per-frame request it always was, behind the admission gate: the frame data of a
 * window request is its LaReq, of a per-frame request the gate's permit (NULL with the gate off) */
static const VSFrame *VS_CC analyseNGetFrameWindows(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    AnalyseNData *d = (AnalyseNData *)inst;
    if (reason == arInitial) {
        if (la_request(&d->la, n, d->super, fd, ctx, vs)) return NULL;
        /* (no slot / no memory: this request takes the per-frame path below) */
    } else if (*fd && *fd != (void *)&d->c.gate) {
        LaReq *r = (LaReq *)*fd;
        *fd = NULL;
        if (reason != arAllFramesReady) { la_release_req(&d->la, r); return NULL; } /* arError */
        LaWindow *s = NULL;
        int rc = la_serve(&d->la, r, &s, ctx, vs);
        const VSFrame *src = vs->getFrameFilter(n, d->super, ctx);
        VSFrame *dst = NULL;
        if (!rc && !src) rc = MVX_E_DEVICE;
        if (!rc) { dst = vs->copyFrame(src, core); rc = multi_set_props(dst, (const char *)s->dblobs + s->dstride * (size_t)(n - s->first), &d->mi, d->fieldSize, vs); }
        shell_quiesce(rc);
        if (src) vs->freeFrame(src);
        la_release_req(&d->la, r);
        if (rc) {
            if (dst) vs->freeFrame(dst);
            if (rc == -1000) vs->setFilterError("AnalyseN: _Field property not found in input frame. Therefore, you must pass tff argument.", ctx);
            else consumer_frame_error(d->c.name, rc, 0, ctx, vs);
            return NULL;
        }
        return dst;
    }
    return consumerGetFrame(n, reason, inst, fd, ctx, core, vs);
}

static void VS_CC analyseNFree(void *inst, VSCore *core, const VSAPI *vs) {
    AnalyseNData *d = (AnalyseNData *)inst;
    if (d->la.on) { la_drain(&d->la); la_close(&d->la, vs); } /* (windows nobody came for are waited for) */
    consumerFree(inst, core, vs);
}

static void VS_CC analyseNCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    static const char *keys[] = { "blksize", "blksizev", "levels", "search", "searchparam", "pelsearch", "isb", "lambda", "chroma", "delta", "truemotion",
                                  "lsad", "plevel", "global", "pnew", "pzero", "pglobal", "overlap", "overlapv", "divide", "badsad", "badrange", "opt",
                                  "meander", "trymany", "fields", "tff", "search_coarse", "dct" };
    mvx_analyse_args a;
    int32_t *av = (int32_t *)&a;
    for (size_t i = 0; i < sizeof(keys) / sizeof(keys[0]); i++) av[i] = opt_int(in, keys[i], vs); /* (isb and delta are not in the argument string: unset) */
    AnalyseNData *d = (AnalyseNData *)consumer_new(sizeof(*d), "AnalyseN", analyseNGetFrameUngated, mvx_analyse_n_destroy_engine);
    char err[1400] = "";
    field_opt(&d->fo, in, vs);
    {
        VSNode *node = vs->mapGetNode(in, "super", 0, NULL);
        const int ok = super_format_ok(vs->getVideoInfo(node));
        vs->freeNode(node);
        if (!ok) snprintf(err, sizeof(err), "AnalyseN: super clip must be GRAY, 420, 422, 440, or 444, up to 16 bits, with constant dimensions.");
    }
    if (!err[0]) d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) {
        d->vi = vs->getVideoInfo(d->super);
        char lerr[MVX_ERRLEN];
        if (mvx_analyse_n_create(&a, (int)vs->mapGetIntSaturated(in, "radius", 0, NULL), d->c.sup, d->vi->numFrames, d->c.geo.pitch, &d->an, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        d->c.engine = d->an;
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    d->mi.radius = (int)vs->mapGetIntSaturated(in, "radius", 0, NULL);
    d->mi.stride = (int64_t)mvx_analyse_n_field_stride(d->an);
    d->fieldSize = mvx_analyse_n_field_size(d->an);
    mvx_analyse_n_get_data(d->an, 0, &d->mi.ad0);
    if (d->c.geo.copies > 1) mvx_analyse_n_set_ref_shadow(d->an, d->c.geo.shadowStride); /* every device super frame of this shell carries its copies */
    pthread_mutex_lock(&g_lock); g_stat_instances++; pthread_mutex_unlock(&g_lock); /* (MVX_VS_STATS=1 reports the shell's thread-seconds for graphs with a searching instance) */
    VSFilterDependency deps[2] = { { d->super, rpGeneral }, { NULL, rpGeneral } };
    int ndeps = 1;
    { /* windows under mv.Analyse's conditions; their length is MVX_VS_MULTI_LOOKAHEAD frames (0 = off), unset the one that puts a Degrain3 graph's chains in flight */
        SuperData *sd = super_lookup(d->super);
        long A = env_long("MVX_VS_LOOKAHEAD", 128);
        if (A > 512) A = 512;
        const long B = getenv("MVX_VS_MULTI_LOOKAHEAD") ? env_long("MVX_VS_MULTI_LOOKAHEAD", 0) : mvx_win_default_length(d->mi.radius, A);
        if (sd && !sd->pelMode && A > 0 && B > 0 && d->vi->numFrames > 1 && cache_cap() > 0) {
            d->la.sd = sd; d->la.owner = d; d->la.numFrames = d->vi->numFrames; d->la.fo = &d->fo; d->la.enqueue = analyse_n_enqueue;
            d->la.before = d->la.after = d->mi.radius; d->la.fixed = -1;
            d->la.frameBytes = 2 * (size_t)d->mi.radius * (size_t)d->mi.stride;
            /* a window pins its frames' and 2 * radius more super frames while it is searched, and its blobs stay in every slot that may be READY */
            la_size(&d->la, B, (double)sd->geo.bytes * 1.2, (double)d->la.frameBytes, LA_SLOTS);
        }
        if (d->la.on) {
            la_open(&d->la, sd->node, vs);
            deps[1].source = d->la.srcNode; ndeps = 2;
        }
    }
    vs->createVideoFilter(out, "AnalyseN", d->vi, d->la.on ? analyseNGetFrameWindows : consumerGetFrame, analyseNFree, fmParallel, deps, ndeps, d, core);
}

/* ---- mv.RecalculateN(super, vectors, ...): the radius is the clip's; one mvx_recalculate_n_frames call per frame */
typedef struct RecalcNData { Consumer c; VSNode *super, *vectors; const VSVideoInfo *vi; mvx_recalculate_n *rn; MultiInfo old, mi; size_t fieldSize; FieldOpt fo; } RecalcNData;

static const VSFrame *VS_CC recalcNGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    RecalcNData *d = (RecalcNData *)inst;
    const int nf = 2 * d->mi.radius;
    if (reason == arInitial) {
        vs->requestFrameFilter(n, d->vectors, ctx);
        vs->requestFrameFilter(n, d->super, ctx);
        multi_request_refs(n, nf, d->vi->numFrames, d->super, ctx, vs);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->super, ctx);
    if (d->fo.fields) { /* src/MVRecalculate.c:121-163: only the error survives, the shift itself never reaches a result */
        int missing = 0;
        frame_top_field(&d->fo, src, n, &missing, vs);
        for (int r = 0; r < nf; r++) {
            const int m = n + multi_offset(r);
            if (m < 0 || m >= d->vi->numFrames) continue;
            const VSFrame *ref = vs->getFrameFilter(m, d->super, ctx);
            frame_top_field(&d->fo, ref, m, &missing, vs);
            vs->freeFrame(ref);
        }
        if (missing) {
            vs->setFilterError("RecalculateN: _Field property not found in input frame. Therefore, you must pass tff argument.", ctx);
            vs->freeFrame(src);
            return NULL;
        }
    }
    const VSFrame *mvn = vs->getFrameFilter(n, d->vectors, ctx);
    void *oldBlob = NULL;
    int rc = multi_to_device(&oldBlob, &d->old, nf, mvn, vs);
    vs->freeFrame(mvn);
    DevRef ds, refs[MULTI_MAX_FIELDS];
    const void *table[MULTI_MAX_FIELDS][3];
    memset(&ds, 0, sizeof(ds)); memset(refs, 0, sizeof(refs)); memset(table, 0, sizeof(table));
    if (!rc) rc = super_to_device(&ds, src, &d->c.geo, vs);
    if (!rc) rc = multi_refs_to_device(refs, table, n, nf, d->vi->numFrames, d->super, &d->c.geo, ctx, vs);
    void *dblob = rc ? NULL : mvx_dev_alloc(2 * (size_t)d->mi.radius * (size_t)d->mi.stride);
    if (!rc && !dblob) rc = MVX_E_NOMEM;
    VSFrame *dst = NULL;
    if (!rc) {
        mvx_recalculate_n_job job;
        memset(&job, 0, sizeof(job));
        for (int p = 0; p < 3; p++) job.src[p] = ds.plane[p];
        job.refs = table; job.old_blob = oldBlob; job.old_field_stride = (size_t)d->old.stride; job.blob = dblob;
        rc = mvx_recalculate_n_frames(d->rn, 1, &job, thread_stream());
        if (!rc) { dst = vs->copyFrame(src, core); rc = multi_set_props(dst, dblob, &d->mi, d->fieldSize, vs); }
    }
    shell_quiesce(rc);
    dev_release(&ds);
    for (int r = 0; r < nf; r++) dev_release(&refs[r]);
    if (dblob) mvx_dev_free(dblob);
    if (oldBlob) mvx_dev_free(oldBlob);
    vs->freeFrame(src);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error(d->c.name, rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

static void VS_CC recalcNCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    static const char *keys[] = { "thsad", "smooth", "blksize", "blksizev", "search", "searchparam", "lambda", "chroma", "truemotion", "pnew", "overlap", "overlapv",
                                  "divide", "meander", "fields", "dct" };
    mvx_recalculate_args a;
    int64_t *av = (int64_t *)&a;
    for (size_t i = 0; i < sizeof(keys) / sizeof(keys[0]); i++) av[i] = opt_int64(in, keys[i], vs);
    RecalcNData *d = (RecalcNData *)consumer_new(sizeof(*d), "RecalculateN", recalcNGetFrameUngated, mvx_recalculate_n_destroy_engine);
    char err[1400] = "";
    field_opt(&d->fo, in, vs);
    d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) { d->vectors = consumer_node(&d->c, in, "vectors", vs); multi_from_clip(&d->old, d->vectors, "RecalculateN", "vectors", err, sizeof(err), vs); }
    if (!err[0]) {
        d->vi = vs->getVideoInfo(d->super);
        char lerr[MVX_ERRLEN];
        if (mvx_recalculate_n_create(&a, d->old.radius, d->c.sup, &d->old.ad0, d->c.geo.pitch, &d->rn, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        d->c.engine = d->rn;
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    d->mi.radius = d->old.radius;
    d->mi.stride = (int64_t)mvx_recalculate_n_field_stride(d->rn);
    d->fieldSize = mvx_recalculate_n_field_size(d->rn);
    mvx_recalculate_n_get_data(d->rn, 0, &d->mi.ad0);
    VSFilterDependency deps[2] = { { d->super, rpGeneral }, { d->vectors, rpStrictSpatial } };
    vs->createVideoFilter(out, "RecalculateN", d->vi, consumerGetFrame, consumerFree, fmParallel, deps, 2, d, core);
}

/* ---- mv.MultiField(vectors, field): one field as an ordinary vector clip (a host copy) */
typedef struct MultiFieldData { Consumer c; VSNode *vectors; MultiInfo mi; mvx_analysis_data ad; int field; } MultiFieldData;

static const VSFrame *VS_CC multiFieldGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    MultiFieldData *d = (MultiFieldData *)inst;
    if (reason == arInitial) { vs->requestFrameFilter(n, d->vectors, ctx); return NULL; }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->vectors, ctx);
    const char *blob = multi_fields_checked(&d->mi, d->field + 1, src, vs);
    VSFrame *dst = NULL;
    if (blob) {
        const char *f = blob + (size_t)d->field * (size_t)d->mi.stride;
        int size = 0;
        memcpy(&size, f, sizeof(size));
        dst = vs->copyFrame(src, core);
        VSMap *props = vs->getFramePropertiesRW(dst);
        vs->mapSetData(props, PROP_ADATA, (const char *)&d->ad, sizeof(d->ad), dtBinary, maReplace);
        vs->mapSetData(props, PROP_VECTORS, f, size, dtBinary, maReplace);
        vs->mapDeleteKey(props, PROP_MULTI_ADATA); vs->mapDeleteKey(props, PROP_MULTI_RADIUS); vs->mapDeleteKey(props, PROP_MULTI_STRIDE); vs->mapDeleteKey(props, PROP_MULTI_VECTORS);
    } else consumer_frame_error(d->c.name, MVX_E_ARG, 0, ctx, vs);
    vs->freeFrame(src);
    return dst;
}

static void VS_CC multiFieldCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    MultiFieldData *d = (MultiFieldData *)consumer_new(sizeof(*d), "MultiField", multiFieldGetFrameUngated, NULL);
    char err[1400] = "";
    d->vectors = consumer_node(&d->c, in, "vectors", vs);
    multi_from_clip(&d->mi, d->vectors, "MultiField", "vectors", err, sizeof(err), vs);
    d->field = (int)vs->mapGetIntSaturated(in, "field", 0, NULL);
    if (!err[0] && (d->field < 0 || d->field >= 2 * d->mi.radius)) snprintf(err, sizeof(err), "MultiField: field must be between 0 and %d.", 2 * d->mi.radius - 1);
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    multi_field_data(&d->ad, &d->mi.ad0, d->field);
    VSFilterDependency deps[1] = { { d->vectors, rpStrictSpatial } };
    vs->createVideoFilter(out, "MultiField", vs->getVideoInfo(d->vectors), consumerGetFrame, consumerFree, fmParallel, deps, 1, d, core);
}

/* ---- mv.DegrainN(clip, super, vectors, radius, ..., thsad2, thsadc2, ..., out16) */
typedef struct DegrainNData { Consumer c; VSNode *node, *super, *vectors; const VSVideoInfo *vi; VSVideoInfo outvi; int radius; mvx_degrain_n *dg; MultiInfo mi; ptrdiff_t pitch[3], dstPitch[3]; } DegrainNData;

static const VSFrame *VS_CC degrainNGetFrameUngated(int n, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    DegrainNData *d = (DegrainNData *)inst;
    const int nr = 2 * d->radius;
    if (reason == arInitial) {
        vs->requestFrameFilter(n, d->vectors, ctx);
        multi_request_refs(n, nr, d->vi->numFrames, d->super, ctx, vs);
        vs->requestFrameFilter(n, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
    const int np = d->vi->format.numPlanes;
    DevRef refs[MULTI_MAX_FIELDS];
    const void *table[MULTI_MAX_FIELDS][3], *blobs[MULTI_MAX_FIELDS];
    memset(refs, 0, sizeof(refs)); memset(table, 0, sizeof(table));
    void *srcArena = NULL, *dstArena = NULL, *dmulti = NULL, *dsrc[3], *ddst[3];
    int height[3] = { 0, 0, 0 };
    for (int p = 0; p < np; p++) height[p] = vs->getFrameHeight(src, p);
    int rc = upload_plane_set(dsrc, &srcArena, src, d->pitch, np, d->vi->format.bytesPerSample, vs);
    if (!rc) rc = dst_plane_set(ddst, &dstArena, d->dstPitch, height, np);
    if (!rc) {
        const VSFrame *vf = vs->getFrameFilter(n, d->vectors, ctx);
        rc = multi_to_device(&dmulti, &d->mi, nr, vf, vs);
        vs->freeFrame(vf);
    }
    if (!rc) rc = multi_refs_to_device(refs, table, n, nr, d->vi->numFrames, d->super, &d->c.geo, ctx, vs);
    if (!rc) {
        mvx_degrain_n_job job;
        memset(&job, 0, sizeof(job));
        for (int p = 0; p < np; p++) { job.src[p] = dsrc[p]; job.dst[p] = ddst[p]; }
        for (int r = 0; r < nr; r++) blobs[r] = (const char *)dmulti + (size_t)r * (size_t)d->mi.stride;
        job.refs = table; job.blobs = blobs;
        rc = mvx_degrain_n_frames(d->dg, 1, &job, thread_stream());
    }
    VSFrame *dst = NULL;
    if (!rc) {
        dst = vs->newVideoFrame(&d->outvi.format, d->outvi.width, d->outvi.height, src, core);
        rc = download_plane_set(dst, ddst, d->dstPitch, np, d->outvi.format.bytesPerSample, vs);
    }
    shell_quiesce(rc);
    for (int r = 0; r < nr; r++) dev_release(&refs[r]);
    if (dmulti) mvx_dev_free(dmulti);
    if (srcArena) mvx_dev_free(srcArena);
    if (dstArena) mvx_dev_free(dstArena);
    vs->freeFrame(src);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error(d->c.name, rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

static void VS_CC degrainNCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    DegrainNData *d = (DegrainNData *)consumer_new(sizeof(*d), "DegrainN", degrainNGetFrameUngated, mvx_degrain_n_destroy_engine);
    char err[1400] = "";
    mvx_degrain_n_args a;
    a.radius = opt_int(in, "radius", vs);
    a.thsad = opt_int64(in, "thsad", vs); a.thsadc = opt_int64(in, "thsadc", vs); a.thsad2 = opt_int64(in, "thsad2", vs); a.thsadc2 = opt_int64(in, "thsadc2", vs);
    a.plane = opt_int(in, "plane", vs); a.limit = opt_int(in, "limit", vs); a.limitc = opt_int(in, "limitc", vs); a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    const int out16 = opt_int(in, "out16", vs) != MVX_UNSET && opt_int(in, "out16", vs) != 0;
    d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) { d->vectors = consumer_node(&d->c, in, "vectors", vs); multi_from_clip(&d->mi, d->vectors, "DegrainN", "vectors", err, sizeof(err), vs); }
    if (!err[0]) {
        if (a.radius == MVX_UNSET) a.radius = d->mi.radius;
        if (a.radius > d->mi.radius) snprintf(err, sizeof(err), "DegrainN: radius is greater than the radius of the vector clip.");
    }
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->vi = vs->getVideoInfo(d->node);
        d->c.floatEntry = 1;
        consumer_check_clip(&d->c, d->vi, vs->getVideoInfo(d->super), 0, err, sizeof(err));
    }
    const int flt = !err[0] && vi_is_float(d->vi);
    if (flt && out16) snprintf(err, sizeof(err), "DegrainN: out16 is not supported on float clips.");
    if (!err[0]) {
        d->outvi = *d->vi;
        if (out16 && !vs->queryVideoFormat(&d->outvi.format, d->vi->format.colorFamily, stInteger, 16, d->vi->format.subSamplingW, d->vi->format.subSamplingH, core))
            snprintf(err, sizeof(err), "DegrainN: the host has no 16 bit format for out16.");
    }
    if (!err[0]) {
        clip_pitches(d->pitch, d->vi, d->vi->format.bytesPerSample);
        clip_pitches(d->dstPitch, &d->outvi, d->outvi.format.bytesPerSample);
        char lerr[MVX_ERRLEN];
        if ((flt ? mvx_degrain_n_create_float : out16 ? mvx_degrain_n_create_out16 : mvx_degrain_n_create)(&a, &d->mi.ad0, d->c.sup, d->pitch, d->c.geo.pitch, d->dstPitch, &d->dg, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        d->c.engine = d->dg;
    }
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    d->radius = a.radius;
    VSFilterDependency deps[3] = { { d->node, rpStrictSpatial }, { d->super, rpGeneral }, { d->vectors, rpStrictSpatial } };
    vs->createVideoFilter(out, "DegrainN", &d->outvi, consumerGetFrame, consumerFree, fmParallel, deps, 3, d, core);
}

/* ---- mv.CompensateN(clip, super, vectors, tr, ...): 2 * tr + 1 output frames per source frame, in temporal order (mvx_compensate_n_map)
 * The first request for any output of source frame n runs ONE mvx_compensate_n_frames job and keeps all 2 * tr + 1 plane sets on the device in a table of the
 * instance; requests for other outputs of the same n wait for it and download their own plane set.  The table is bounded (MVX_VS_MULTI_SETS, default 8 sets),
 * its bytes count against the device cache's budget, and the least recently used idle set makes room; an evicted set is computed again.  What a frame holds never
 * depends on which request computed its set. */
enum { CS_EMPTY, CS_BUILDING, CS_READY };
typedef struct CompSet { int n, state, users; uint64_t stamp; void *arena; } CompSet;
#define COMP_SETS_MAX 64
typedef struct CompNData {
    Consumer c; VSNode *node, *super, *vectors; const VSVideoInfo *clipvi; VSVideoInfo vi; mvx_compensate_n *cn; MultiInfo mi; int tr, no;
    ptrdiff_t pitch[3]; int height[3]; size_t planeOff[3], frameBytes;
    pthread_mutex_t mu; pthread_cond_t cv; CompSet sets[COMP_SETS_MAX]; int nsets; uint64_t stamp;
} CompNData;

static void comp_sets_account(size_t bytes, int add) { /* the table shares the device budget of the frame cache */
    pthread_mutex_lock(&g_lock);
    if (add) g_cache_bytes += bytes; else g_cache_bytes -= bytes;
    pthread_mutex_unlock(&g_lock);
}
/* all outputs of source frame n into `arena` */
static int comp_n_build(CompNData *d, int n, void *arena, VSFrameContext *ctx, const VSAPI *vs) {
    const int nf = 2 * d->tr, np = d->clipvi->format.numPlanes;
    DevRef ds, refs[MULTI_MAX_FIELDS];
    const void *table[MULTI_MAX_FIELDS][3];
    void *dst[MULTI_MAX_FIELDS + 1][3];
    memset(&ds, 0, sizeof(ds)); memset(refs, 0, sizeof(refs)); memset(table, 0, sizeof(table)); memset(dst, 0, sizeof(dst));
    void *dmulti = NULL;
    const VSFrame *vf = vs->getFrameFilter(n, d->vectors, ctx);
    int rc = multi_to_device(&dmulti, &d->mi, nf, vf, vs);
    vs->freeFrame(vf);
    if (!rc) rc = clip_super_to_device(&ds, n, d->super, &d->c.geo, ctx, vs);
    if (!rc) rc = multi_refs_to_device(refs, table, n, nf, d->clipvi->numFrames, d->super, &d->c.geo, ctx, vs);
    if (!rc) {
        for (int k = 0; k < d->no; k++) for (int p = 0; p < np; p++) dst[k][p] = (char *)arena + (size_t)k * d->frameBytes + d->planeOff[p];
        mvx_compensate_n_job job;
        memset(&job, 0, sizeof(job));
        for (int p = 0; p < 3; p++) job.src_super[p] = ds.plane[p];
        job.refs = table; job.blob = dmulti; job.field_stride = (size_t)d->mi.stride; job.dst = dst;
        rc = mvx_compensate_n_frames(d->cn, 1, &job, thread_stream());
        if (!rc) rc = mvx_stream_sync(thread_stream()); /* the other requests of this set download on their own streams */
    }
    shell_quiesce(rc);
    dev_release(&ds);
    for (int r = 0; r < nf; r++) dev_release(&refs[r]);
    if (dmulti) mvx_dev_free(dmulti);
    return rc;
}
/* the set of source frame n, computed if the table does not hold it: *held is the table's entry (give it back with comp_set_release) or NULL with *own an arena of the
 * caller's (every entry was in use) */
static int comp_set_acquire(CompNData *d, int n, CompSet **held, void **own, VSFrameContext *ctx, const VSAPI *vs) {
    *held = NULL; *own = NULL;
    CompSet *s = NULL;
    pthread_mutex_lock(&d->mu);
    for (;;) {
        s = NULL;
        for (int i = 0; i < d->nsets; i++) if (d->sets[i].state != CS_EMPTY && d->sets[i].n == n) s = &d->sets[i];
        if (!s) break;
        if (s->state == CS_READY) { s->users++; s->stamp = ++d->stamp; pthread_mutex_unlock(&d->mu); *held = s; return 0; }
        pthread_cond_wait(&d->cv, &d->mu); /* being built: GPU work only, nothing it waits for needs a host worker thread */
    }
    for (int i = 0; i < d->nsets && !s; i++) if (d->sets[i].state == CS_EMPTY) s = &d->sets[i];
    if (!s) for (int i = 0; i < d->nsets; i++) if (d->sets[i].state == CS_READY && d->sets[i].users == 0 && (!s || d->sets[i].stamp < s->stamp)) s = &d->sets[i];
    if (s) { s->state = CS_BUILDING; s->n = n; s->users = 1; s->stamp = ++d->stamp; }
    pthread_mutex_unlock(&d->mu);
    const size_t bytes = (size_t)d->no * d->frameBytes;
    void *arena = s ? s->arena : NULL;
    if (!arena) {
        arena = shell_alloc(bytes);
        if (arena && s) { s->arena = arena; comp_sets_account(bytes, 1); }
    }
    const int rc = arena ? comp_n_build(d, n, arena, ctx, vs) : MVX_E_NOMEM;
    if (s) {
        pthread_mutex_lock(&d->mu);
        if (rc) { s->state = CS_EMPTY; s->users = 0; } else s->state = CS_READY; /* (a failed set is nobody's: whoever waited for it computes it itself and reports its own error) */
        pthread_cond_broadcast(&d->cv);
        pthread_mutex_unlock(&d->mu);
        if (!rc) *held = s;
    } else if (rc) { if (arena) mvx_dev_free(arena); }
    else *own = arena;
    return rc;
}
static void comp_set_release(CompNData *d, CompSet *held, void *own) {
    if (held) { pthread_mutex_lock(&d->mu); held->users--; pthread_mutex_unlock(&d->mu); }
    if (own) mvx_dev_free(own);
}

static const VSFrame *VS_CC compNGetFrameUngated(int m, int reason, void *inst, void **fd, VSFrameContext *ctx, VSCore *core, const VSAPI *vs) {
    (void)fd;
    CompNData *d = (CompNData *)inst;
    const int n = m / d->no, k = m % d->no;
    if (reason == arInitial) { /* everything the set needs: whichever request of source frame n comes first computes all of its outputs */
        vs->requestFrameFilter(n, d->vectors, ctx);
        vs->requestFrameFilter(n, d->super, ctx);
        multi_request_refs(n, 2 * d->tr, d->clipvi->numFrames, d->super, ctx, vs);
        vs->requestFrameFilter(n, d->node, ctx);
        return NULL;
    }
    if (reason != arAllFramesReady) return NULL;
    const int np = d->clipvi->format.numPlanes;
    CompSet *held = NULL;
    void *own = NULL;
    int rc = comp_set_acquire(d, n, &held, &own, ctx, vs);
    VSFrame *dst = NULL;
    if (!rc) {
        const VSFrame *src = vs->getFrameFilter(n, d->node, ctx);
        dst = vs->newVideoFrame(&d->vi.format, d->vi.width, d->vi.height, src, core);
        vs->freeFrame(src);
        void *planes[3] = { NULL, NULL, NULL };
        for (int p = 0; p < np; p++) planes[p] = (char *)(held ? held->arena : own) + (size_t)k * d->frameBytes + d->planeOff[p];
        rc = download_plane_set(dst, planes, d->pitch, np, d->vi.format.bytesPerSample, vs);
        shell_quiesce(rc);
    }
    comp_set_release(d, held, own);
    if (rc) {
        if (dst) vs->freeFrame(dst);
        consumer_frame_error(d->c.name, rc, 0, ctx, vs);
        return NULL;
    }
    return dst;
}

static void VS_CC compNFree(void *inst, VSCore *core, const VSAPI *vs) {
    CompNData *d = (CompNData *)inst;
    for (int i = 0; i < d->nsets; i++) if (d->sets[i].arena) { comp_sets_account((size_t)d->no * d->frameBytes, 0); mvx_dev_free(d->sets[i].arena); }
    pthread_mutex_destroy(&d->mu); pthread_cond_destroy(&d->cv);
    consumerFree(inst, core, vs);
}

static void VS_CC compNCreate(const VSMap *in, VSMap *out, void *user, VSCore *core, const VSAPI *vs) {
    warm_barrier();
    (void)user;
    CompNData *d = (CompNData *)consumer_new(sizeof(*d), "CompensateN", compNGetFrameUngated, mvx_compensate_n_destroy_engine);
    char err[1400] = "";
    mvx_compensate_args a;
    a.scbehavior = opt_int(in, "scbehavior", vs); a.thsad = opt_int64(in, "thsad", vs); a.thscd1 = opt_int64(in, "thscd1", vs); a.thscd2 = opt_int(in, "thscd2", vs);
    a.time = opt_float(in, "time", 100.0, vs);
    { FieldOpt fo; field_opt(&fo, in, vs); a.fields = fo.fields; } /* (fields = 1 is the library's to refuse; tff has nothing to act on) */
    int tr = opt_int(in, "tr", vs);
    d->super = consumer_super(&d->c, in, err, sizeof(err), vs);
    if (!err[0]) { d->vectors = consumer_node(&d->c, in, "vectors", vs); multi_from_clip(&d->mi, d->vectors, "CompensateN", "vectors", err, sizeof(err), vs); }
    if (!err[0]) {
        if (tr == MVX_UNSET) tr = d->mi.radius;
        if (tr > d->mi.radius) snprintf(err, sizeof(err), "CompensateN: tr is greater than the radius of the vector clip.");
    }
    if (!err[0]) {
        d->node = consumer_node(&d->c, in, "clip", vs);
        d->clipvi = vs->getVideoInfo(d->node);
        d->c.floatEntry = 1;
        consumer_check_clip(&d->c, d->clipvi, vs->getVideoInfo(d->super), 1, err, sizeof(err));
    }
    if (!err[0]) {
        clip_pitches(d->pitch, d->clipvi, d->clipvi->format.bytesPerSample);
        char lerr[MVX_ERRLEN];
        if ((vi_is_float(d->clipvi) ? mvx_compensate_n_create_float : mvx_compensate_n_create)(&a, tr, &d->mi.ad0, d->c.sup, d->c.geo.pitch, d->pitch, &d->cn, lerr)) snprintf(err, sizeof(err), "%s", lerr);
        d->c.engine = d->cn;
    }
    if (!err[0] && (int64_t)d->clipvi->numFrames * (2 * tr + 1) > 2147483647LL) snprintf(err, sizeof(err), "CompensateN: the output clip would have too many frames.");
    if (err[0]) { consumer_fail(&d->c, err, out, vs); return; }
    d->tr = tr; d->no = 2 * tr + 1;
    for (int p = 0; p < d->clipvi->format.numPlanes; p++) {
        d->height[p] = p ? d->clipvi->height >> d->clipvi->format.subSamplingH : d->clipvi->height;
        d->planeOff[p] = d->frameBytes;
        d->frameBytes += (size_t)d->pitch[p] * (size_t)d->height[p];
    }
    pthread_mutex_init(&d->mu, NULL); pthread_cond_init(&d->cv, NULL);
    d->nsets = (int)env_long("MVX_VS_MULTI_SETS", 8);
    if (d->nsets < 1) d->nsets = 1;
    if (d->nsets > COMP_SETS_MAX) d->nsets = COMP_SETS_MAX;
    d->vi = *d->clipvi;
    d->vi.numFrames = d->clipvi->numFrames * d->no;
    d->vi.fpsNum = d->clipvi->fpsNum * d->no;
    VSFilterDependency deps[3] = { { d->node, rpGeneral }, { d->super, rpGeneral }, { d->vectors, rpGeneral } };
    vs->createVideoFilter(out, "CompensateN", &d->vi, consumerGetFrame, compNFree, fmParallel, deps, 3, d, core);
    if (d->vi.fpsNum > 0 && d->vi.fpsDen > 0) assume_fps(out, "CompensateN", d->vi.fpsNum, d->vi.fpsDen, core, vs);
}

/* ------------------------------------------------------------------------------------------------ entry point */

#define DEGRAIN_TAIL "thsad:int:opt;thsadc:int:opt;plane:int:opt;limit:int:opt;limitc:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;"

/* replaces src/EntryPoint.c:28-52 for the filters of the hot path */
VS_EXTERNAL_API(void) VapourSynthPluginInit2(VSPlugin *plugin, const VSPLUGINAPI *vspapi) {
    /* (the search streams want GPU_MAX_HW_QUEUES >= 12 -- see search_stream_next.  That is a setting of the HOST PROCESS, read once when the HIP
     * runtime initialises: a plugin must not change the process environment behind its host's back, so it is documented in INTEGRATION.md and set
     * by the mini host / the launch scripts, not here.  r6: an unconfigured host is TOLD once, under MVX_VS_STATS, that its searches will share
     * the runtime's default four hardware queues) */
    if (env_long("MVX_VS_STATS", 0)) {
        const char *q = getenv("GPU_MAX_HW_QUEUES");
        if (!q || atoi(q) < SEARCH_STREAMS)
            fprintf(stderr, "mvtools (MI355X): GPU_MAX_HW_QUEUES is %s: the %d search streams of concurrent mv.Analyse instances share the HIP runtime's hardware queues and "
                            "serialise; export GPU_MAX_HW_QUEUES=16 before starting the host (INTEGRATION.md)\n", q ? q : "unset (runtime default: 4)", SEARCH_STREAMS);
    }
    /* r6: the HIP runtime, this library's code objects and the page-locked staging buffers come up on a background thread while the host is still reading its
     * script / opening its clips: 0.3 s + 0.1 s + ~20 ms per buffer that the first frames (mv.DegrainN's creation reads frame 0 of every vector clip) no longer wait for.
     * (see warmup_thread) */
    if (env_long("MVX_VS_WARMUP", 1)) {
        if (!__atomic_load_n(&g_warm_started, __ATOMIC_ACQUIRE)) {
            __atomic_store_n(&g_warm_started, 1, __ATOMIC_RELEASE);
            if (pthread_create(&g_warm_thread, NULL, warmup_thread, NULL) != 0) __atomic_store_n(&g_warm_started, 0, __ATOMIC_RELEASE);
        }
    }
    vspapi->configPlugin("com.nodame.mvtools", "mv", "MVTools v24", VS_MAKE_VERSION(24, 0), VS_MAKE_VERSION(VAPOURSYNTH_API_MAJOR, VAPOURSYNTH_API_MINOR), 0, plugin);
    vspapi->registerFunction("Super",
                             "clip:vnode;hpad:int:opt;vpad:int:opt;pel:int:opt;levels:int:opt;chroma:int:opt;sharp:int:opt;rfilter:int:opt;pelclip:vnode:opt;opt:int:opt;",
                             "clip:vnode;", superCreate, NULL, plugin);
    vspapi->registerFunction("Analyse",
                             "super:vnode;blksize:int:opt;blksizev:int:opt;levels:int:opt;search:int:opt;searchparam:int:opt;pelsearch:int:opt;isb:int:opt;lambda:int:opt;"
                             "chroma:int:opt;delta:int:opt;truemotion:int:opt;lsad:int:opt;plevel:int:opt;global:int:opt;pnew:int:opt;pzero:int:opt;pglobal:int:opt;"
                             "overlap:int:opt;overlapv:int:opt;divide:int:opt;badsad:int:opt;badrange:int:opt;opt:int:opt;meander:int:opt;trymany:int:opt;fields:int:opt;"
                             "tff:int:opt;search_coarse:int:opt;dct:int:opt;",
                             "clip:vnode;", analyseCreate, NULL, plugin);
    vspapi->registerFunction("Finest", "super:vnode;opt:int:opt;", "clip:vnode;", finestCreate, NULL, plugin);
    vspapi->registerFunction("SCDetection", "clip:vnode;vectors:vnode;thscd1:int:opt;thscd2:int:opt;", "clip:vnode;", scdCreate, NULL, plugin);
    vspapi->registerFunction("Recalculate",
                             "super:vnode;vectors:vnode;thsad:int:opt;smooth:int:opt;blksize:int:opt;blksizev:int:opt;search:int:opt;searchparam:int:opt;lambda:int:opt;"
                             "chroma:int:opt;truemotion:int:opt;pnew:int:opt;overlap:int:opt;overlapv:int:opt;divide:int:opt;opt:int:opt;meander:int:opt;fields:int:opt;"
                             "tff:int:opt;dct:int:opt;",
                             "clip:vnode;", recalcCreate, NULL, plugin);
    vspapi->registerFunction("Degrain1", "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;" DEGRAIN_TAIL, "clip:vnode;", degrainCreate, (void *)(intptr_t)1, plugin);
    vspapi->registerFunction("Degrain2", "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;mvbw2:vnode;mvfw2:vnode;" DEGRAIN_TAIL, "clip:vnode;", degrainCreate, (void *)(intptr_t)2, plugin);
    vspapi->registerFunction("Degrain3", "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;mvbw2:vnode;mvfw2:vnode;mvbw3:vnode;mvfw3:vnode;" DEGRAIN_TAIL, "clip:vnode;", degrainCreate, (void *)(intptr_t)3, plugin);
    vspapi->registerFunction("Degrain4", "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;mvbw2:vnode;mvfw2:vnode;mvbw3:vnode;mvfw3:vnode;mvbw4:vnode;mvfw4:vnode;" DEGRAIN_TAIL, "clip:vnode;", degrainCreate, (void *)(intptr_t)4, plugin);
    vspapi->registerFunction("Degrain5", "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;mvbw2:vnode;mvfw2:vnode;mvbw3:vnode;mvfw3:vnode;mvbw4:vnode;mvfw4:vnode;mvbw5:vnode;mvfw5:vnode;" DEGRAIN_TAIL, "clip:vnode;", degrainCreate, (void *)(intptr_t)5, plugin);
    vspapi->registerFunction("Degrain6", "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;mvbw2:vnode;mvfw2:vnode;mvbw3:vnode;mvfw3:vnode;mvbw4:vnode;mvfw4:vnode;mvbw5:vnode;mvfw5:vnode;mvbw6:vnode;mvfw6:vnode;" DEGRAIN_TAIL, "clip:vnode;", degrainCreate, (void *)(intptr_t)6, plugin);
    vspapi->registerFunction("BlockFPS",
                             "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;num:int:opt;den:int:opt;mode:int:opt;ml:float:opt;blend:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",
                             "clip:vnode;", fpsCreate, NULL, plugin);
    vspapi->registerFunction("Compensate",
                             "clip:vnode;super:vnode;vectors:vnode;scbehavior:int:opt;thsad:int:opt;fields:int:opt;time:float:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;tff:int:opt;",
                             "clip:vnode;", compCreate, NULL, plugin);
    /* dct 1..4 are opt-in in the library (mvx_enable_dct_float): MVX_VS_DCT=1, read here, once, switches them on for this process.   */
    if (env_long("MVX_VS_DCT", 0)) (void)mvx_enable_dct_float(1);
    /* 32-bit float clips, by a switch of its own, read the same way: MVX_VS_FLOAT=1.  It registers nothing: mv.Super and the filters with a float entry in the library
     * (Compensate, BlockFPS; DegrainN, CompensateN; FlowInter, FlowFPS, Flow, FlowBlur; DepanCompensate, DepanStabilise -- each behind its family's switch) then take a
     * float clip, and every other filter refuses one.   */
    g_vs_float = env_long("MVX_VS_FLOAT", 0) != 0;
    /* The per-sample filters are opt-in for now: MVX_VS_FLOW=1 in the host's environment when the plugin is loaded (read here, once).  Without it the
     * plugin registers exactly the functions above.   */
    if (env_long("MVX_VS_FLOW", 0)) {
        vspapi->registerFunction("FlowInter",
                                 "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;time:float:opt;ml:float:opt;blend:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",
                                 "clip:vnode;", flowCreate, NULL, plugin);
        vspapi->registerFunction("FlowFPS",
                                 "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;num:int:opt;den:int:opt;mask:int:opt;ml:float:opt;blend:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",
                                 "clip:vnode;", flowCreate, (void *)(intptr_t)1, plugin);
        vspapi->registerFunction("Flow",
                                 "clip:vnode;super:vnode;vectors:vnode;time:float:opt;mode:int:opt;fields:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;tff:int:opt;",
                                 "clip:vnode;", flowCompCreate, NULL, plugin);
        vspapi->registerFunction("FlowBlur",
                                 "clip:vnode;super:vnode;mvbw:vnode;mvfw:vnode;blur:float:opt;prec:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",
                                 "clip:vnode;", blurCreate, NULL, plugin);
        vspapi->registerFunction("Mask",
                                 "clip:vnode;vectors:vnode;ml:float:opt;gamma:float:opt;kind:int:opt;time:float:opt;ysc:int:opt;thscd1:int:opt;thscd2:int:opt;opt:int:opt;",
                                 "clip:vnode;", maskCreate, NULL, plugin);
        /* mv.Mask for clips of 9 to 16 bits is a switch of its own beside this one, read the same way: MVX_VS_MASK_DEEP=1.   */
        g_mask_deep = env_long("MVX_VS_MASK_DEEP", 0) != 0;
    }
    /* The Depan family is opt-in by a switch of its own, read the same way: MVX_VS_DEPAN=1.  (src/MVDepan.cpp:4211-4288) */
    if (env_long("MVX_VS_DEPAN", 0)) {
        vspapi->registerFunction("DepanAnalyse",
                                 "clip:vnode;vectors:vnode;mask:vnode:opt;zoom:int:opt;rot:int:opt;pixaspect:float:opt;error:float:opt;info:int:opt;wrong:float:opt;zerow:float:opt;"
                                 "thscd1:int:opt;thscd2:int:opt;fields:int:opt;tff:int:opt;",
                                 "clip:vnode;", depanAnalyseCreate, NULL, plugin);
        vspapi->registerFunction("DepanEstimate",
                                 "clip:vnode;trust:float:opt;winx:int:opt;winy:int:opt;wleft:int:opt;wtop:int:opt;dxmax:int:opt;dymax:int:opt;zoommax:float:opt;stab:float:opt;"
                                 "pixaspect:float:opt;info:int:opt;show:int:opt;fields:int:opt;tff:int:opt;",
                                 "clip:vnode;", depanEstimateCreate, NULL, plugin);
        vspapi->registerFunction("DepanCompensate",
                                 "clip:vnode;data:vnode;offset:float:opt;subpixel:int:opt;pixaspect:float:opt;matchfields:int:opt;mirror:int:opt;blur:int:opt;info:int:opt;fields:int:opt;"
                                 "tff:int:opt;",
                                 "clip:vnode;", depanCompCreate, NULL, plugin);
        vspapi->registerFunction("DepanStabilise",
                                 "clip:vnode;data:vnode;cutoff:float:opt;damping:float:opt;initzoom:float:opt;addzoom:int:opt;prev:int:opt;next:int:opt;mirror:int:opt;blur:int:opt;"
                                 "dxmax:float:opt;dymax:float:opt;zoommax:float:opt;rotmax:float:opt;subpixel:int:opt;pixaspect:float:opt;fitlast:int:opt;tzoom:float:opt;info:int:opt;"
                                 "method:int:opt;fields:int:opt;",
                                 "clip:vnode;", depanStabCreate, NULL, plugin);
    }
    /* The temporal-radius filters over the multi vector clip, by a switch of their own, read the same way: MVX_VS_MULTI=1.   */
    if (env_long("MVX_VS_MULTI", 0)) {
        vspapi->registerFunction("AnalyseN",
                                 "super:vnode;radius:int;blksize:int:opt;blksizev:int:opt;levels:int:opt;search:int:opt;searchparam:int:opt;pelsearch:int:opt;lambda:int:opt;"
                                 "chroma:int:opt;truemotion:int:opt;lsad:int:opt;plevel:int:opt;global:int:opt;pnew:int:opt;pzero:int:opt;pglobal:int:opt;"
                                 "overlap:int:opt;overlapv:int:opt;divide:int:opt;badsad:int:opt;badrange:int:opt;opt:int:opt;meander:int:opt;trymany:int:opt;fields:int:opt;"
                                 "tff:int:opt;search_coarse:int:opt;dct:int:opt;",
                                 "clip:vnode;", analyseNCreate, NULL, plugin);
        vspapi->registerFunction("RecalculateN",
                                 "super:vnode;vectors:vnode;thsad:int:opt;smooth:int:opt;blksize:int:opt;blksizev:int:opt;search:int:opt;searchparam:int:opt;lambda:int:opt;"
                                 "chroma:int:opt;truemotion:int:opt;pnew:int:opt;overlap:int:opt;overlapv:int:opt;divide:int:opt;opt:int:opt;meander:int:opt;fields:int:opt;"
                                 "tff:int:opt;dct:int:opt;",
                                 "clip:vnode;", recalcNCreate, NULL, plugin);
        vspapi->registerFunction("DegrainN",
                                 "clip:vnode;super:vnode;vectors:vnode;radius:int:opt;thsad:int:opt;thsadc:int:opt;thsad2:int:opt;thsadc2:int:opt;plane:int:opt;limit:int:opt;limitc:int:opt;"
                                 "thscd1:int:opt;thscd2:int:opt;out16:int:opt;",
                                 "clip:vnode;", degrainNCreate, NULL, plugin);
        vspapi->registerFunction("CompensateN",
                                 "clip:vnode;super:vnode;vectors:vnode;tr:int:opt;scbehavior:int:opt;thsad:int:opt;fields:int:opt;time:float:opt;thscd1:int:opt;thscd2:int:opt;tff:int:opt;",
                                 "clip:vnode;", compNCreate, NULL, plugin);
        vspapi->registerFunction("MultiField", "vectors:vnode;field:int;", "clip:vnode;", multiFieldCreate, NULL, plugin);
    }
}
