// seen_ratio_cli — the reference's `seen_ratio` experiment (eee/src/seen_ratio.rs:16-29) as a plain C++ program over the C ABI of
// libtakzero_hip.so: for each ply 0 .. plies-1, `games` fresh games from the openings play that many uniformly random legal moves on
// the device (tz_search_random_steps) and the hash net says which share of the positions it has not seen (tz_search_hash_seen).
// The model's bitvec.bin is read from beside it.  Prints the reference's text: `random = [`, `    (ply, ratio),` per ply, `]`.
// Game g of ply p has the id p * games + g; its opening choice is drawn from its key with the counter 0xFFFFFFFF
// (takzero_amd/eee.py makes the same games).
//
//   g++ -std=c++17 -O2 examples/seen_ratio_cli.cpp -Iinclude -Ltakzero_amd -ltakzero_hip -Wl,-rpath,$PWD/takzero_amd -o seen_ratio_cli
//   ./seen_ratio_cli --model model_1200000.ot --arch net4_lcghash [--games 65536 --plies 100 --batch 4096 --seed 123]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "arch_arg.h"
#include "takzero_hip.h"

#define CHECK(call)                                                        \
    do {                                                                   \
        if ((call) != 0) {                                                 \
            fprintf(stderr, "%s failed: %s\n", #call, tz_last_error());    \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// splitmix64's finaliser, the library's counter-based draw (csrc/tz_math.h)
static uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the shortest decimal that reads back as the same float, as Rust's `{}` prints an f32
static std::string shortest(float v) {
    char buf[32];
    for (int p = 1; p <= 9; p++) {
        snprintf(buf, sizeof buf, "%.*g", p, v);
        if (strtof(buf, nullptr) == v) break;
    }
    return buf;
}

int main(int argc, char** argv) {
    std::string model;
    int arch = TZ_ARCH_NET4_LCGHASH, games = 65536, plies = 100, batch = 4096, device = 0, half_komi = 4;
    unsigned long long seed = 123;
    auto usage = []() {
        fprintf(stderr, "usage: seen_ratio_cli --model PATH.ot --arch net4_lcghash|net4_simhash|net6_simhash [--games 65536 --plies 100 "
                        "--batch 4096 --seed 123 --half-komi 4 --device G]\n");
        return 2;
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--model") model = next();
        else if (a == "--arch") arch = arch_from_arg(next());
        else if (a == "--games") games = atoi(next());
        else if (a == "--plies") plies = atoi(next());
        else if (a == "--batch") batch = atoi(next());
        else if (a == "--seed") seed = strtoull(next(), nullptr, 10);
        else if (a == "--half-komi") half_komi = atoi(next());
        else if (a == "--device") device = atoi(next());
        else return usage();
    }
    if (model.empty() || arch < 0 || !arch_has_set(arch) || games <= 0 || plies < 0 || batch <= 0) return usage();
    const int n = arch_board(arch);
    batch = std::min(batch, games);

    tz_net* net = nullptr;
    tz_search* search = nullptr;
    CHECK(tz_net_create(n, arch, device, TZ_PREC_F16, 0, &net));
    CHECK(tz_net_load_weights(net, model.c_str()));   // and bitvec.bin beside it
    CHECK(tz_search_create(net, TZ_AGENT_NET, batch, n, half_komi, 1, &search));   // a playout uses no tree beyond the root slot

    std::vector<int32_t> choice(batch);
    std::vector<uint8_t> seen(batch);
    const uint64_t key = mix64(seed);
    printf("random = [\n");
    for (int ply = 0; ply < plies; ply++) {
        long long unseen = 0;
        for (int lo = 0; lo < games; lo += batch) {
            const int count = std::min(batch, games - lo);
            const uint64_t game_base = (uint64_t)ply * (uint64_t)games + (uint64_t)lo;
            for (int g = 0; g < batch; g++) choice[g] = (int32_t)(mix64(mix64(key ^ (game_base + g)) ^ 0xFFFFFFFFull) % 16);
            CHECK(tz_search_new_openings(search, choice.data()));
            CHECK(tz_search_random_steps(search, seed, game_base, ply, 0, nullptr, nullptr, nullptr));
            CHECK(tz_search_hash_seen(search, seen.data()));
            for (int g = 0; g < count; g++) unseen += seen[g] ? 0 : 1;
        }
        printf("    (%d, %s),\n", ply, shortest((float)((double)unseen / games)).c_str());
        fflush(stdout);
    }
    printf("]\n");
    tz_search_destroy(search);
    tz_net_destroy(net);
    return 0;
}
