/* The arithmetic of the shell's look-ahead windows (mvtools_vs.c), free of the device and of the host's API so that it can be tested on its own
 * (tests/vs_window_main.c).  A vector clip is computed a WINDOW of B consecutive frames at a time: window v holds the frames [v * B, v * B + B) that lie
 * inside the clip and needs the super frames of those plus `before` frames in front of them and `after` frames behind them, as far as the clip has them.
 * mv.Analyse has before or after = delta (forward or backward); mv.AnalyseN has both = radius. */
#ifndef MVX_VS_WINDOW_H
#define MVX_VS_WINDOW_H

/* chains a Degrain3 graph puts in flight per look-ahead window of mv.Analyse's default length: six clips of 128 frames */
#define MVX_WIN_CHAINS 768
#define MVX_WIN_MIN 8

/* mv.AnalyseN's window length when MVX_VS_MULTI_LOOKAHEAD is unset: as many frames as put MVX_WIN_CHAINS chains (2 * radius per frame) in flight, at least
 * MVX_WIN_MIN and at most mv.Analyse's own length (MVX_VS_LOOKAHEAD); where that is below MVX_WIN_MIN it wins */
static inline int mvx_win_default_length(int radius, long lookahead) {
    long b = MVX_WIN_CHAINS / (2 * (radius < 1 ? 1 : radius));
    if (b < MVX_WIN_MIN) b = MVX_WIN_MIN;
    if (b > lookahead) b = lookahead;
    return (int)b;
}

/* the window of frame n, and the slot of window w in a table of `slots` */
static inline int mvx_win_of(int n, int B) { return n / B; }
static inline int mvx_win_slot(int w, int slots) { return w % slots; }

/* window v of a clip of numFrames: its frames [*first, *first + *count) and the source frames [*lo, *hi] it needs */
static inline void mvx_win_inputs(int v, int B, int numFrames, int before, int after, int *first, int *count, int *lo, int *hi) {
    const int f = v * B, last = (f + B < numFrames ? f + B : numFrames) - 1;
    *first = f; *count = last - f + 1;
    *lo = f - before > 0 ? f - before : 0;
    *hi = last + after < numFrames ? last + after : numFrames - 1;
}

/* the order of the fields of a multi blob: mvbw1, mvfw1, mvbw2, mvfw2, ...  Frame n + mvx_win_field_offset(r) is the reference of field r ... */
static inline int mvx_win_field_offset(int r) { return r % 2 == 0 ? r / 2 + 1 : -(r / 2 + 1); }
/* ... and this is its place among the inputs [lo, hi] of the window that holds frame n, or -1 for a reference the window has not (outside the clip) */
static inline int mvx_win_field_input(int n, int r, int lo, int hi) {
    const int m = n + mvx_win_field_offset(r);
    return m < lo || m > hi ? -1 : m - lo;
}

/* device bytes the windows of one instance may hold at a time: the window being consumed and `depth` windows ahead pin B + extra super frames each (extra = before + after),
 * and each of `slots` windows keeps B frames' vectors until its slot is recycled */
static inline double mvx_win_bytes(int B, int depth, int extra, double superBytes, double blobBytes, int slots) {
    return (double)(depth + 1) * (double)(B + extra) * superBytes + (double)slots * (double)B * blobBytes;
}
/* makes that fit `avail`: first fewer windows ahead, then shorter windows (halved while longer than MVX_WIN_MIN).  0: not even that fits -- the per-frame path */
static inline int mvx_win_fit(int *B, int *depth, int extra, double superBytes, double blobBytes, int slots, double avail) {
    while (*depth > 0 && mvx_win_bytes(*B, *depth, extra, superBytes, blobBytes, slots) > avail) (*depth)--;
    while (*B > MVX_WIN_MIN && mvx_win_bytes(*B, *depth, extra, superBytes, blobBytes, slots) > avail) *B /= 2;
    return mvx_win_bytes(*B, *depth, extra, superBytes, blobBytes, slots) <= avail;
}

#endif
