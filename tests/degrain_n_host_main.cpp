// Stand-alone host program around csrc/mvx_degrain_n_weights.h, the header the device code of mv.DegrainN takes its weight arithmetic from
// (test infrastructure; tests/test_degrain_n_host.py builds it, optionally with -fsanitize=address,undefined, and compares its output with
// the Python restatement).  It reads commands from the file named by argv[1], one per line, and answers each with one line:
//
//   weights N th_0 .. th_{N-1} usable_0 .. usable_{N-1} sad_0 .. sad_{N-1}   ->  WSrc W_0 .. W_{N-1}
//       the list form of the plan kernel: the references whose weight is not 0 are collected, WSum summed, the list normalised in place
//   table t1 t2 radius nSCD1 nSCD1_old                                       ->  over t_1 .. t_radius   (scaled thresholds per distance)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "mvx_degrain_n_weights.h"

struct Entry { int r, w; };

static int weights(FILE *f) {
    int n;
    if (fscanf(f, "%d", &n) != 1 || n < 1 || n > DN_MAX_REFS) return 1;
    std::vector<long long> th(n), sad(n);
    std::vector<int> usable(n);
    for (int r = 0; r < n; r++) if (fscanf(f, "%lld", &th[r]) != 1) return 1;
    for (int r = 0; r < n; r++) if (fscanf(f, "%d", &usable[r]) != 1) return 1;
    for (int r = 0; r < n; r++) if (fscanf(f, "%lld", &sad[r]) != 1) return 1;
    std::vector<Entry> list;
    int WSum = dn_wsum_begin();
    for (int r = 0; r < n; r++) {
        if (!usable[r]) continue;
        const int w = dn_weight(th[r], sad[r]);
        if (w == 0) continue;
        list.push_back(Entry{r, w});
        WSum += w;
    }
    const double scale = dn_scale(WSum);
    int WSrc = 256;
    std::vector<int> out(n, 0);
    for (Entry &e : list) { e.w = dn_scaled(e.w, scale); WSrc -= e.w; out[e.r] = e.w; }
    printf("%d", WSrc);
    for (int r = 0; r < n; r++) printf(" %d", out[r]);
    printf("\n");
    return 0;
}

static int table(FILE *f) {
    long long t1, t2, s1, s1old;
    int radius;
    if (fscanf(f, "%lld %lld %d %lld %lld", &t1, &t2, &radius, &s1, &s1old) != 5 || radius < 1 || radius > DN_MAX_RADIUS) return 1;
    int64_t t[DN_MAX_RADIUS];
    const int over = dn_threshold_table(t1, t2, radius, s1, s1old, t);
    printf("%d", over);
    for (int d = 0; d < radius; d++) printf(" %lld", (long long)t[d]);
    printf("\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: degrain_n_host_main COMMANDS\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char cmd[16];
    int rc = 0;
    while (!rc && fscanf(f, "%15s", cmd) == 1) {
        if (!strcmp(cmd, "weights")) rc = weights(f);
        else if (!strcmp(cmd, "table")) rc = table(f);
        else rc = 1;
    }
    fclose(f);
    if (rc) { fprintf(stderr, "degrain_n_host_main: malformed command file\n"); return 1; }
    printf("degrain_n_host_main: ok\n");
    return 0;
}
