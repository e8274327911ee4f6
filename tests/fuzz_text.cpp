// Sanitizer fuzz of the native text entry points (tz_parse_targets / tz_format_targets, host code only):
// mutated target lines in exact-size heap buffers under AddressSanitizer + UBSan.  Built and run by tests/test_fuzz_text.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "takzero_hip.h"
// A target line with exactly amax moves round-trips in every byte; one with amax + 1 moves is skipped and counted, the line after it
// is still parsed, and consumed_out covers all three.  All buffers are exact-size heap blocks: the row of the accepted line ends where
// its allocation ends, and the row the refused line was being parsed into is the last one of its allocation (max_targets = 2).
static int capacity_case(int n, int amax) {
    const char* tps = n == 3 ? "x3/x,1,x/2,x2 1 2" : n == 4 ? "x4/x,1,x2/x4/2,x3 1 2" : n == 5 ? "x5/x5/x2,1,x2/x5/2,x4 1 2"
                                                                                               : "x6/x6/x2,1,x3/x6/x6/2,x5 1 2";
    const int half_komi = n == 3 ? 0 : 4, wide = amax + 1, size = tz_policy_size(n);
    tz_state s;
    if (tz_state_from_tps(tps, n, half_komi, &s)) return 1;
    std::vector<uint16_t> mv(wide);
    std::vector<float> pol(wide);
    for (int k = 0; k < wide; k++) {                       // every move of the board size in turn (3x3 has 243: they repeat)
        mv[k] = (uint16_t)((k * 7) % size);
        pol[k] = (float)(k % 97 + 1) / 1024.0f;
    }
    const float value = -0.25f, ube = 1.5f;
    int32_t nm = amax;
    std::vector<char> out((size_t)3 * (400 + 32 * wide));
    uint64_t w = 0;
    if (tz_format_targets(n, 1, &s, mv.data(), pol.data(), &nm, amax, &value, &ube, out.data(), out.size(), &w)) return 2;
    const std::string full(out.data(), w);
    nm = wide;
    if (tz_format_targets(n, 1, &s, mv.data(), pol.data(), &nm, wide, &value, &ube, out.data(), out.size(), &w)) return 3;
    const std::string over(out.data(), w);
    const std::string text = full + over + full;
    char* buf = (char*)malloc(text.size());
    memcpy(buf, text.data(), text.size());
    const int maxt = 2;
    tz_state* st = (tz_state*)malloc(maxt * sizeof(tz_state));
    uint16_t* pm = (uint16_t*)malloc((size_t)maxt * amax * sizeof(uint16_t));
    float* pp = (float*)malloc((size_t)maxt * amax * sizeof(float));
    int32_t pn[maxt];
    float pv[maxt], pu[maxt];
    int32_t cnt = 0, skp = 0;
    uint64_t used = 0;
    int rc = tz_parse_targets(buf, text.size(), n, half_komi, maxt, amax, st, pm, pp, pn, pv, pu, &cnt, &used, &skp);
    int bad = 0;
    if (rc != 0 || cnt != 2 || skp != 1 || used != text.size()) bad = 4;
    for (int t = 0; !bad && t < 2; t++) {
        if (pn[t] != amax || pv[t] != value || pu[t] != ube || memcmp(&st[t], &s, sizeof s)) bad = 5;
        if (memcmp(pm + (size_t)t * amax, mv.data(), amax * sizeof(uint16_t)) || memcmp(pp + (size_t)t * amax, pol.data(), amax * sizeof(float))) bad = 6;
    }
    if (!bad) {
        if (tz_format_targets(n, 2, st, pm, pp, pn, amax, pv, pu, out.data(), out.size(), &w)) bad = 7;
        else if (std::string(out.data(), w) != full + full) bad = 8;
    }
    if (bad) printf("capacity case n=%d amax=%d: check %d failed (rc=%d count=%d skipped=%d consumed=%llu of %llu)\n", n, amax, bad, rc, cnt, skp,
                    (unsigned long long)used, (unsigned long long)text.size());
    free(buf);
    free(st);
    free(pm);
    free(pp);
    return bad;
}

int main(int argc, char** argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 20000;
    const int pairs[4][2] = {{3, 512}, {4, 512}, {5, 512}, {6, 1024}};     // the (n, amax) the native learn loop parses with
    for (auto& p : pairs)
        if (capacity_case(p[0], p[1])) return 1;
    const int n = 5, amax = 512, maxt = 64;
    std::vector<tz_state> st(maxt);
    std::vector<uint16_t> mv(maxt * amax);
    std::vector<float> pol(maxt * amax), val(maxt), ube(maxt);
    std::vector<int32_t> nm(maxt);
    std::string base = "x2,1221,x,1S/2,2C,2,1,x/x,212,21C,2S,2/2211S,2,21,1,1/x2,221S,2,x 2 23;0.5;1.25;a1:0.25,Sb2:0.5,3c3>12:0.25\n";
    std::mt19937 rng(1);
    long parsed = 0, skipped_total = 0;
    for (int it = 0; it < iterations; it++) {
        std::string s;
        int lines = 1 + rng() % 3;
        for (int l = 0; l < lines; l++) {
            std::string x = base;
            int muts = rng() % 4;
            for (int m = 0; m < muts; m++) {
                size_t p = rng() % x.size();
                switch (rng() % 4) {
                    case 0: x[p] = (char)(rng() % 256); break;
                    case 1: x.erase(p, 1 + rng() % 5); break;
                    case 2: x.insert(p, std::string(1 + rng() % 3, ";:,x/1S"[rng() % 7])); break;
                    case 3: x = x.substr(0, p); break;
                }
                if (x.empty()) x = "\n";
            }
            s += x;
        }
        int32_t cnt = 0, skp = 0;
        uint64_t used = 0;
        // exact-size heap copy so that any over-read is caught
        char* buf = (char*)malloc(s.size());
        memcpy(buf, s.data(), s.size());
        int rc = tz_parse_targets(buf, s.size(), n, 4, maxt, amax, st.data(), mv.data(), pol.data(), nm.data(), val.data(), ube.data(), &cnt, &used, &skp);
        free(buf);
        if (rc != 0 || used > s.size() || cnt < 0 || cnt > maxt) { printf("bad rc=%d used=%llu\n", rc, (unsigned long long)used); return 1; }
        parsed += cnt; skipped_total += skp;
        if (cnt > 0) {  // whatever parsed must format again
            std::vector<char> out(cnt * (200 + 32 * amax));
            uint64_t w = 0;
            rc = tz_format_targets(n, cnt, st.data(), mv.data(), pol.data(), nm.data(), amax, val.data(), ube.data(), out.data(), out.size(), &w);
            if (rc != 0) { printf("format rc=%d: %s\n", rc, tz_last_error()); return 1; }
        }
    }
    printf("ok parsed=%ld skipped=%ld\n", parsed, skipped_total);
    return 0;
}
