// tei_cli — the reference's `tei` binary (tei/src/main.rs) as a plain C++ program over the C ABI of libtakzero_hip.so: a UCI-style
// text engine that a Tak GUI or a bot can drive.  The handshake (main.rs:36-137) is here; everything after `readyok` is the engine
// session of the library (tz_tei_*, include/takzero_hip.h section "tei"): one tree, tree reuse over `position`, `go` on
// Node::simulate_batch.  A reader thread queues the input lines and calls tz_tei_stop at once for `stop` and `quit`; the main
// thread feeds tz_tei_line and prints what comes back; info lines are printed as they arise.  What the reference logs goes to stderr.
//
//   g++ -std=c++17 -O2 -pthread examples/tei_cli.cpp -Iinclude -Ltakzero_amd -ltakzero_hip -Wl,-rpath,$PWD/takzero_amd -o tei_cli
//   ./tei_cli --arch net6_simhash [--half-komi 4 --leaves 128 --node-capacity 8388608 --selection puct --device 0]
//   > tei / setoption name model value model_latest.ot / isready / position startpos moves a1 f6 / go movetime 2000
// (--arch test takes --n and --blocks; --seed X starts from Net::new(seed) when no model is set.)
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "arch_arg.h"
#include "selection_arg.h"
#include "takzero_hip.h"

static const int MAX_ERRORS_IN_A_ROW = 5;  // main.rs:23

struct Lines {
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::string> q;
    void push(const std::string& s) {
        {
            std::lock_guard<std::mutex> g(m);
            q.push_back(s);
        }
        cv.notify_one();
    }
    std::string pop() {
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return !q.empty(); });
        std::string s = q.front();
        q.pop_front();
        return s;
    }
};

static std::string first_word(const std::string& line) {
    const size_t a = line.find_first_not_of(" \t\r\n\v\f");
    if (a == std::string::npos) return "";
    const size_t b = line.find_first_of(" \t\r\n\v\f", a);
    return line.substr(a, b == std::string::npos ? std::string::npos : b - a);
}

static int print_info(void*, const char* line) {
    printf("%s\n", line);
    fflush(stdout);
    return 0;
}

int main(int argc, char** argv) {
    std::string selection = "puct";
    int arch = -1, n = 5, blocks = 0, leaves = 128, precision = TZ_PREC_F16, device = 0, half_komi = 4, node_capacity = 8388608;
    bool have_seed = false;
    unsigned long long seed = 0;
    auto usage = []() {
        fprintf(stderr, "usage: tei_cli --arch 4|5|6|14|24|34|100|net4_simhash|net5|net6_simhash|net4_lcghash|net4_ensemble|net4_rnd|test [--n N --blocks K "
                        "--half-komi 4 --leaves 128 --node-capacity 8388608 --selection puct|uct|improved --seed X --device G --f32|--bf16]\n");
        return 2;
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--arch") arch = arch_from_arg(next());
        else if (a == "--n") n = atoi(next());
        else if (a == "--blocks") blocks = atoi(next());
        else if (a == "--half-komi") half_komi = atoi(next());
        else if (a == "--leaves") leaves = atoi(next());
        else if (a == "--node-capacity") node_capacity = atoi(next());
        else if (a == "--selection") selection = next();
        else if (a == "--seed") seed = strtoull(next(), nullptr, 10), have_seed = true;
        else if (a == "--device") device = atoi(next());
        else if (a == "--f32") precision = TZ_PREC_F32;
        else if (a == "--bf16") precision = TZ_PREC_BF16;
        else return usage();
    }
    if (arch < 0 || selection_rule(selection) < 0) return usage();
    if (arch_board(arch)) n = arch_board(arch);

    int kind = 0, n_moves = 0;
    int64_t numbers[8];
    char text[4096];
    std::string line;
    // the reference's get_input: one trimmed line, parsed (main.rs:320-324)
    auto get_input = [&]() -> int {
        if (!std::getline(std::cin, line)) {
            fprintf(stderr, "reading from stdin failed\n");
            return TZ_EINVAL;
        }
        const int rc = tz_tei_parse(line.c_str(), n, &kind, numbers, nullptr, 0, &n_moves, text, (int)sizeof text);
        if (rc == TZ_EPARSE) fprintf(stderr, "%s\n", tz_last_error());
        return rc == TZ_EPARSE ? rc : TZ_OK;  // a `position` with moves does not fit here, and is not expected here
    };

    if (get_input() != TZ_OK || kind != TZ_TEI_TEI) {  // main.rs:36-40
        fprintf(stderr, "first message received should be `tei`\n");
        return 1;
    }
    printf("id name TakZero-HIP\n");
    printf("id author the takzero_amd contributors\n");
    printf("option name model type string default ./path/to/model.ot\n");
    printf("option name HalfKomi type combo default %d var %d\n", half_komi, half_komi);
    printf("teiok\n");
    fflush(stdout);

    std::string model;
    for (;;) {  // main.rs:66-91
        const int rc = get_input();
        if (rc == TZ_EINVAL) return 1;  // end of input
        if (rc) continue;
        if (kind == TZ_TEI_ISREADY) break;
        if (kind == TZ_TEI_SETOPTION) {
            const std::string t = text, name = t.substr(0, t.find(' ')), value = t.substr(t.find(' ') + 1);
            if (name == "model") {
                model = value;
            } else if (name == "HalfKomi") {
                char* end = nullptr;
                const long k = strtol(value.c_str(), &end, 10);
                if (value.empty() || *end) {
                    fprintf(stderr, "could not parse half komi\n");
                    return 1;
                }
                if (k != half_komi) {
                    fprintf(stderr, "half komi of %ld was requested, but only %d is supported\n", k, half_komi);
                    return 1;
                }
            } else {
                fprintf(stderr, "unknown option: %s\n", name.c_str());
            }
        } else {
            fprintf(stderr, "only expecting `isready` or `option` messages\n");
        }
    }
    if (model.empty() && !have_seed) {
        fprintf(stderr, "model path must be set\n");
        return 1;
    }

    tz_net* net = nullptr;
    tz_search* search = nullptr;
    tz_tei* tei = nullptr;
    auto fail = [&](const char* what) {
        fprintf(stderr, "%s: %s\n", what, tz_last_error());
        return 1;
    };
    if (tz_net_create(n, arch, device, precision, blocks, &net)) return fail("tz_net_create");
    if (tz_net_init_random(net, seed)) return fail("tz_net_init_random");  // Net::load_partial starts from Net::new (network/mod.rs:30-35)
    if (!model.empty()) {
        int n_missing = 0;
        if (tz_net_load_partial(net, model.c_str(), text, (int)sizeof text, &n_missing)) return fail("failed to load model");
        if (n_missing) fprintf(stderr, "%d tensors are not in the model file and keep their initial values\n", n_missing);
    }
    if (tz_search_create(net, TZ_AGENT_NET, 1, n, half_komi, node_capacity, &search)) return fail("tz_search_create");
    if (tz_search_set_selection(search, selection_rule(selection))) return fail("tz_search_set_selection");
    if (tz_tei_create(search, leaves, &tei)) return fail("tz_tei_create");
    tz_tei_set_sink(tei, print_info, nullptr);

    Lines lines;
    std::thread reader([&lines, tei]() {
        std::string l;
        for (;;) {
            if (!std::getline(std::cin, l)) l = "quit";  // the end of the input ends the program
            const std::string w = first_word(l);
            if (w == "stop" || w == "quit") tz_tei_stop(tei);
            lines.push(l);
            if (w == "quit") return;
        }
    });
    printf("readyok\n");
    fflush(stdout);

    std::vector<char> out(1 << 20);
    int errors_in_a_row = 0, status = 0;
    bool reader_done = false;
    for (;;) {
        const std::string l = lines.pop();
        reader_done = first_word(l) == "quit";
        uint64_t size = 0;
        int quit = 0;
        const int rc = tz_tei_line(tei, l.c_str(), out.data(), out.size(), &size, &quit);
        // the library's `info string error / warning` lines are the reference's log: to stderr with the rest of it
        for (char* p = out.data(); *p;) {
            char* e = strchr(p, '\n');
            const std::string one(p, e ? (size_t)(e - p) : strlen(p));
            if (one.rfind("info string error: ", 0) == 0 || one.rfind("info string warning: ", 0) == 0) fprintf(stderr, "%s\n", one.c_str() + 12);
            else printf("%s\n", one.c_str());
            if (!e) break;
            p = e + 1;
        }
        fflush(stdout);
        if (rc == TZ_EPARSE) {
            if (++errors_in_a_row >= MAX_ERRORS_IN_A_ROW) {  // main.rs:118-131
                fprintf(stderr, "there were %d errors in a row\n", MAX_ERRORS_IN_A_ROW);
                status = 1;
                break;
            }
            continue;
        }
        errors_in_a_row = 0;
        if (rc && rc != TZ_ESTATE) {
            fprintf(stderr, "%s\n", tz_last_error());
            if (rc == TZ_EDEVICE || rc == TZ_ENOMEM) status = 1;
        }
        if (quit || status) break;
    }
    if (reader_done) {
        reader.join();  // it has seen `quit` or the end of the input
    } else {
        reader.detach();  // it may sit in a read that never returns, and it names the session: the process ends under it
        fflush(stdout);
        fflush(stderr);
        _Exit(status);
    }
    tz_tei_destroy(tei);
    tz_search_destroy(search);
    tz_net_destroy(net);
    return status;
}
