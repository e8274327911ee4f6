// analysis_cli — the search of the reference's `analysis` binary (analysis/src/main.rs:32-82) as a plain C++ program over the C ABI
// of libtakzero_hip.so: one tree, Node::simulate_batch with BATCH_SIZE leaves per network call (tz_search_simulate_batch, beta 0),
// then what the reference prints of the node: root visits and evaluation, the children sorted by visits, and the principal
// variation in PTN.  One position per run (--tps, default the empty board); there is no REPL.
//
//   g++ -std=c++17 -O2 examples/analysis_cli.cpp -Iinclude -Ltakzero_amd -ltakzero_hip -Wl,-rpath,$PWD/takzero_amd -o analysis_cli
//   ./analysis_cli --model model_latest.ot --arch 5 --tps "x5/x5/x5/x5/x5 1 1" [--leaves 128 --rounds 8]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "arch_arg.h"
#include "selection_arg.h"
#include "takzero_hip.h"

#define CHECK(call)                                                        \
    do {                                                                   \
        if ((call) != 0) {                                                 \
            fprintf(stderr, "%s failed: %s\n", #call, tz_last_error());    \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static std::string eval_text(uint8_t tag, uint32_t bits) {
    char buf[48];
    if (tag == TZ_EVAL_VALUE) {
        float v;
        memcpy(&v, &bits, 4);
        snprintf(buf, sizeof buf, "%+.4f", v);
    } else {
        snprintf(buf, sizeof buf, "%s(%u)", tag == TZ_EVAL_WIN ? "Win" : tag == TZ_EVAL_LOSS ? "Loss" : "Draw", bits);
    }
    return buf;
}

int main(int argc, char** argv) {
    std::string model, tps, selection = "puct";
    int arch = TZ_ARCH_NET5, n = 5, blocks = 0, leaves = 128, rounds = 8, precision = TZ_PREC_F16, device = 0, half_komi = 4, show = 10;
    unsigned long long seed = 0;
    auto usage = []() {
        fprintf(stderr, "usage: analysis_cli [--model FILE.ot|.tzw --tps TPS --arch 4|5|6|14|24|34|100|net4_simhash|net5|net6_simhash|net4_lcghash|net4_ensemble|net4_rnd|test --n N --blocks K --leaves 128 --rounds 8 --selection puct|uct|improved "
                        "--half-komi 4 --children 10 --seed X --device G --f32|--bf16]\n");
        return 2;
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--model") model = next();
        else if (a == "--tps") tps = next();
        else if (a == "--arch") arch = arch_from_arg(next());
        else if (a == "--n") n = atoi(next());
        else if (a == "--blocks") blocks = atoi(next());
        else if (a == "--leaves") leaves = atoi(next());
        else if (a == "--selection") selection = next();
        else if (a == "--rounds") rounds = atoi(next());
        else if (a == "--half-komi") half_komi = atoi(next());
        else if (a == "--children") show = atoi(next());
        else if (a == "--seed") seed = strtoull(next(), nullptr, 10);
        else if (a == "--device") device = atoi(next());
        else if (a == "--f32") precision = TZ_PREC_F32;
        else if (a == "--bf16") precision = TZ_PREC_BF16;
        else return usage();
    }
    if (selection_rule(selection) < 0) return usage();
    if (arch_board(arch)) n = arch_board(arch);
    tz_net* net = nullptr;
    tz_search* search = nullptr;
    CHECK(tz_net_create(n, arch, device, precision, blocks, &net));
    if (!model.empty()) CHECK(tz_net_load_weights(net, model.c_str()));
    else CHECK(tz_net_init_random(net, seed));
    CHECK(tz_search_create(net, TZ_AGENT_NET, 1, n, half_komi, 0, &search));
    CHECK(tz_search_set_selection(search, selection_rule(selection)));
    if (!tps.empty()) {
        tz_state start;
        const int32_t game = 0;
        CHECK(tz_state_from_tps(tps.c_str(), n, half_komi, &start));
        CHECK(tz_search_set_positions(search, 1, &game, &start));
    }
    tz_state pos;
    char text[512];
    CHECK(tz_search_get_positions(search, &pos));
    CHECK(tz_state_to_tps(&pos, text, sizeof text));
    printf("tps: %s\n", text);

    const float beta = 0.0f;  // analysis/src/main.rs:16
    CHECK(tz_search_simulate_batch(search, &beta, leaves, rounds));

    int amax = 0;
    CHECK(tz_search_shape(search, nullptr, nullptr, nullptr, &amax));
    tz_root_info root;
    std::vector<uint16_t> moves(amax);
    std::vector<uint32_t> visits(amax), bits(amax);
    std::vector<uint8_t> tags(amax);
    std::vector<float> prob(amax);
    CHECK(tz_search_root_info(search, &root));
    CHECK(tz_search_root_children(search, amax, moves.data(), visits.data(), tags.data(), bits.data(), nullptr, prob.data(), nullptr));
    printf("visits: %u\n", root.visit_count);
    printf("evaluation: %s\n", eval_text(root.eval_tag, root.eval.ply).c_str());
    std::vector<int> order(root.n_children);
    for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return visits[a] > visits[b]; });
    for (int i = 0; i < (int)order.size() && i < show; i++) {
        const int c = order[i];
        CHECK(tz_move_to_ptn(n, moves[c], text, sizeof text));
        printf("child: %s visits %u evaluation %s policy %.4f\n", text, visits[c], eval_text(tags[c], bits[c]).c_str(), prob[c]);
    }
    std::vector<uint16_t> pv(512);
    int len = 0;
    CHECK(tz_search_principal_variation(search, 0, pv.data(), (int)pv.size(), &len));
    printf("pv:");
    for (int i = 0; i < len && i < (int)pv.size(); i++) {
        CHECK(tz_move_to_ptn(n, pv[i], text, sizeof text));
        printf(" %s", text);
    }
    printf("\n");
    tz_search_destroy(search);
    tz_net_destroy(net);
    return 0;
}
