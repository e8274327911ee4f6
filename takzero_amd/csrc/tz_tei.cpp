// tz_tei.cpp — the reference's `tei` binary above the search ABI, in native host code: Input::from_str and Output::Info's Display
// (tei/src/protocol.rs:74-160, 240-274) and the session of tei/src/main.rs:139-297 (one tree, tree reuse over `position`, the
// `go` loop on Node::simulate_batch, clock and node limits).  Everything goes through the public C ABI of the search
// (include/takzero_hip.h, section "tei", which also lists where the session leaves the reference); examples/tei_cli.cpp is the
// program around it.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tz_engine.h"
#include "tz_math.h"

namespace {

constexpr float BETA = 0.0f;            // tei/src/main.rs:27
constexpr int INFO_INTERVAL_MS = 300;   // DURATION_BETWEEN_INFO_PRINTS, main.rs:24

std::vector<std::string> split_words(const char* s) {  // str::split_whitespace
    std::vector<std::string> out;
    std::string cur;
    for (; *s; s++) {
        const unsigned char c = (unsigned char)*s;
        if (c == ' ' || (c >= 9 && c <= 13)) {
            if (!cur.empty()) out.push_back(cur);
            cur.clear();
        } else {
            cur += (char)c;
        }
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

// str::parse::<u64 / usize>: an optional '+', then decimal digits only, no overflow
bool parse_u64(const std::string& w, uint64_t* out) {
    size_t i = !w.empty() && w[0] == '+' ? 1 : 0;
    if (i == w.size()) return false;
    uint64_t v = 0;
    for (; i < w.size(); i++) {
        if (w[i] < '0' || w[i] > '9') return false;
        const uint64_t d = (uint64_t)(w[i] - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

struct Parsed {
    int kind = TZ_TEI_ERROR;
    int64_t numbers[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint16_t> moves;
    std::string text;  // TPS, or "<name> <value>"
    int err = 0;
    std::string err_text;
};

int parse_fail(Parsed& p, int err, const std::string& text) {
    p.kind = TZ_TEI_ERROR;
    p.err = err;
    p.err_text = text;
    p.numbers[0] = err;
    return TZ_EPARSE;
}

// Input::from_str, protocol.rs:74-160
int parse_line(const char* line, int n, Parsed& p) {
    const std::vector<std::string> w = split_words(line);
    size_t i = 0;
    auto next = [&]() -> const std::string* { return i < w.size() ? &w[i++] : nullptr; };
    const std::string* first = next();
    if (!first) return parse_fail(p, TZ_TEI_ERR_MISSING_FIRST_WORD, "missing first word");
    if (*first == "tei") {
        p.kind = TZ_TEI_TEI;
    } else if (*first == "isready") {
        p.kind = TZ_TEI_ISREADY;
    } else if (*first == "stop") {
        p.kind = TZ_TEI_STOP;
    } else if (*first == "quit") {
        p.kind = TZ_TEI_QUIT;
    } else if (*first == "setoption") {
        const char* missing_name = "missing `name` or the actual option name after `option`";
        const std::string* a = next();
        if (!a || *a != "name") return parse_fail(p, TZ_TEI_ERR_MISSING_NAME, missing_name);
        const std::string* name = next();
        if (!name) return parse_fail(p, TZ_TEI_ERR_MISSING_NAME, missing_name);
        const std::string* b = next();
        if (!b || *b != "value")
            return parse_fail(p, TZ_TEI_ERR_MISSING_VALUE, "missing `value` or the actual value after `option name <id>`");
        const std::string* value = next();
        if (!value) return parse_fail(p, TZ_TEI_ERR_MISSING_NAME, missing_name);  // protocol.rs:97 names MissingName here
        p.kind = TZ_TEI_SETOPTION;
        p.text = *name + " " + *value;
    } else if (*first == "teinewgame") {
        const std::string* a = next();
        if (!a) return parse_fail(p, TZ_TEI_ERR_MISSING_SIZE, "missing size after `newgame`");
        uint64_t size = 0;
        if (!parse_u64(*a, &size)) return parse_fail(p, TZ_TEI_ERR_PARSE_INT, "new game size parse error: invalid number '" + *a + "'");
        p.kind = TZ_TEI_NEWGAME;
        p.numbers[0] = (int64_t)size;
    } else if (*first == "position") {
        const std::string* a = next();
        if (!a) return parse_fail(p, TZ_TEI_ERR_MISSING_POSITION, "missing second word after `position`");
        if (*a == "startpos") {
            p.numbers[0] = 0;
        } else if (*a == "tps") {
            const std::string *pos = next(), *player = next(), *number = next();
            if (!pos || !player || !number) return parse_fail(p, TZ_TEI_ERR_MISSING_TPS, "missing TPS after `position tps`");
            p.text = *pos + " " + *player + " " + *number;
            tz_state st;
            uint64_t move_number = 0;
            if ((*player != "1" && *player != "2") || !parse_u64(*number, &move_number) || move_number == 0 ||
                tz_state_from_tps(p.text.c_str(), n, 0, &st) != TZ_OK)
                return parse_fail(p, TZ_TEI_ERR_PARSE_TPS, "position tps parse error: '" + p.text + "' is not a TPS of this board size");
            p.numbers[0] = 1;
        } else {
            return parse_fail(p, TZ_TEI_ERR_UNRECOGNIZED, "unrecognized option");
        }
        const std::string* m = next();
        if (m && *m == "moves") {
            while (const std::string* mv = next()) {
                uint16_t idx = 0;
                if (tz_move_from_ptn(n, mv->c_str(), &idx) != TZ_OK)
                    return parse_fail(p, TZ_TEI_ERR_PARSE_MOVE, "move parse error: '" + *mv + "'");
                p.moves.push_back(idx);
            }
        }
        p.kind = TZ_TEI_POSITION;
    } else if (*first == "go") {
        while (const std::string* word = next()) {
            int opt;
            if (*word == "wtime") opt = TZ_TEI_GO_WTIME;
            else if (*word == "btime") opt = TZ_TEI_GO_BTIME;
            else if (*word == "winc") opt = TZ_TEI_GO_WINC;
            else if (*word == "binc") opt = TZ_TEI_GO_BINC;
            else if (*word == "movetime") opt = TZ_TEI_GO_MOVETIME;
            else if (*word == "nodes") opt = TZ_TEI_GO_NODES;
            else if (*word == "infinite") opt = TZ_TEI_GO_INFINITE;
            else return parse_fail(p, TZ_TEI_ERR_UNRECOGNIZED, "unrecognized option");
            if (opt != TZ_TEI_GO_INFINITE) {
                const std::string* v = next();
                if (!v)
                    return opt == TZ_TEI_GO_NODES ? parse_fail(p, TZ_TEI_ERR_MISSING_AMOUNT, "missing the amount of nodes after `go nodes`")
                                                  : parse_fail(p, TZ_TEI_ERR_MISSING_SECONDS, "missing seconds after time parameter in `go`");
                uint64_t x = 0;
                if (!parse_u64(*v, &x) || x > (uint64_t)INT64_MAX)
                    return parse_fail(p, TZ_TEI_ERR_PARSE_INT, "new game size parse error: invalid number '" + *v + "'");
                p.numbers[1 + opt] = (int64_t)x;  // a repeated option: the last one holds (main.rs:217-236)
            }
            p.numbers[0] |= (int64_t)1 << opt;
        }
        p.kind = TZ_TEI_GO;
    } else {
        return parse_fail(p, TZ_TEI_ERR_UNRECOGNIZED, "unrecognized option");
    }
    return TZ_OK;
}

// impl From<Eval> for f32, eval.rs:95-105
float eval_to_f32(uint8_t tag, uint32_t bits) {
    if (tag == TZ_EVAL_VALUE) return tz_bits_to_float(bits);
    const float base = tz_powif(TZ_DISCOUNT, (int)bits);
    return base * (tag == TZ_EVAL_WIN ? 1.0f : tag == TZ_EVAL_LOSS ? -1.0f : 0.0f);
}

// f32::round() as i32: halves away from zero; the cast saturates and sends NaN to 0
int round_to_i32(float x) {
    const float r = roundf(x);
    if (r != r) return 0;
    if (r >= 2147483648.0f) return INT32_MAX;
    if (r <= -2147483648.0f) return INT32_MIN;
    return (int)r;
}

// Output::Info's Display, protocol.rs:240-274
int format_info(int n, uint64_t time_ms, uint64_t nodes, uint8_t tag, uint32_t bits, const uint16_t* pv, int pv_len, std::string& o) {
    char buf[128];
    const float score = eval_to_f32(tag, bits);
    const int centipawns = round_to_i32(score * 100.0f);
    // the reference divides by zero at 0 ms (and its product wraps where this one gives way to the quotient first)
    const uint64_t nps = !time_ms ? 0 : nodes > UINT64_MAX / 1000 ? nodes / time_ms * 1000 : 1000 * nodes / time_ms;
    snprintf(buf, sizeof buf, "info time %llu nodes %llu nps %llu", (unsigned long long)time_ms, (unsigned long long)nodes,
             (unsigned long long)nps);
    o = buf;
    if (tag == TZ_EVAL_WIN) {
        o += " wdl 1000 0 0";
    } else if (tag == TZ_EVAL_LOSS) {
        o += " wdl 0 0 1000";
    } else if (tag == TZ_EVAL_DRAW) {
        o += " wdl 0 1000 0";
    } else {
        const int per_mille = 500 + round_to_i32(score * 500.0f);
        snprintf(buf, sizeof buf, " wdl %d 0 %d", per_mille, 1000 - per_mille);
        o += buf;
    }
    if (tag == TZ_EVAL_WIN || tag == TZ_EVAL_LOSS) {
        snprintf(buf, sizeof buf, " score mate %s%u", tag == TZ_EVAL_LOSS ? "-" : "", bits / 2 + bits % 2);
        o += buf;
    }
    snprintf(buf, sizeof buf, " score cp %d", centipawns);
    o += buf;
    o += " pv";
    for (int i = 0; i < pv_len; i++) {
        int rc = tz_move_to_ptn(n, pv[i], buf, sizeof buf);
        if (rc) return rc;
        o += " ";
        o += buf;
    }
    return TZ_OK;
}

}  // namespace

struct tz_tei {
    tz_search* s = nullptr;
    int leaves = 128, n = 0, half_komi = 0, max_actions = 0;
    int info_interval_ms = INFO_INTERVAL_MS;
    int (*sink)(void*, const char*) = nullptr;
    void* sink_user = nullptr;
    // tz_tei_stop from the reader thread against the stop / quit lines handled by tz_tei_line
    std::atomic<uint64_t> stops_announced{0};
    uint64_t stop_lines = 0;
    // last_position / last_moves, main.rs:154-155
    bool have_last = false;
    std::string last_position;  // "" = startpos, else the canonical TPS
    std::vector<uint16_t> last_moves;
};

namespace {

std::string ptn(const tz_tei* t, uint16_t mv) {
    char buf[64];
    return tz_move_to_ptn(t->n, mv, buf, sizeof buf) == TZ_OK ? std::string(buf) : "?";
}

int start_state(const tz_tei* t, tz_state* out) {  // Env::default()
    std::string tps;
    for (int r = 0; r < t->n; r++) tps += (r ? "/x" : "x") + std::to_string(t->n);
    tps += " 1 1";
    return tz_state_from_tps(tps.c_str(), t->n, t->half_komi, out);
}

int reset_to(tz_tei* t, const tz_state& st) {
    const int32_t game = 0;
    return tz_search_set_positions(t->s, 1, &game, &st);
}

// one move of a `position` replay; *legal = 0: not playable here (the position and tree are as before)
int play_move(tz_tei* t, uint16_t mv, bool keep_tree, int* legal) {
    int rc;
    *legal = 0;
    tz_root_info root;
    if ((rc = tz_search_root_info(t->s, &root))) return rc;
    if (keep_tree && root.n_children > 0) {
        std::vector<uint16_t> moves(root.n_children);
        if ((rc = tz_search_root_children(t->s, (int)root.n_children, moves.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)))
            return rc;
        bool among = false;
        for (uint16_t m : moves) among = among || m == mv;
        if (!among) return TZ_OK;
        *legal = 1;
        return tz_search_step_wide(t->s, &mv);
    }
    int8_t ok = 0;  // Node::descend on a childless node leaves a default node: validate, play, reset the tree
    if ((rc = tz_search_play_moves(t->s, &mv, &ok))) return rc;
    *legal = ok == 1;
    return TZ_OK;
}

int on_position(tz_tei* t, const Parsed& p, std::string& out) {
    int rc;
    std::string position;
    tz_state st;
    if (p.numbers[0] == 1) {
        char buf[512];
        if ((rc = tz_state_from_tps(p.text.c_str(), t->n, t->half_komi, &st))) return rc;
        if ((rc = tz_state_to_tps(&st, buf, sizeof buf))) return rc;
        position = buf;
    } else if ((rc = start_state(t, &st))) {
        return rc;
    }
    const bool reuse = t->have_last && position == t->last_position && p.moves.size() >= t->last_moves.size() &&
                       std::equal(t->last_moves.begin(), t->last_moves.end(), p.moves.begin());  // main.rs:175
    size_t from = 0;
    if (reuse) {
        from = t->last_moves.size();
    } else if ((rc = reset_to(t, st))) {
        return rc;
    }
    bool all_played = true;
    for (size_t i = from; i < p.moves.size(); i++) {
        int legal = 0;
        if ((rc = play_move(t, p.moves[i], reuse, &legal))) return rc;
        if (!legal) {
            out += "info string error: could not play move " + ptn(t, p.moves[i]) + "\n";  // main.rs:180-183, 193-196
            all_played = false;
            break;
        }
    }
    // the reference remembers the list even when its replay stopped early; the next `position` would then extend a list that
    // was never played, so it is forgotten here and the next one starts afresh
    t->have_last = all_played;
    t->last_position = position;
    t->last_moves = p.moves;
    return TZ_OK;
}

int emit_info(tz_tei* t, uint64_t ms, uint64_t visits, const tz_root_info& root, std::string& out, bool* stop) {
    int rc, len = 0;
    std::vector<uint16_t> pv(512);
    if ((rc = tz_search_principal_variation(t->s, 0, pv.data(), (int)pv.size(), &len))) return rc;
    std::string line;
    if ((rc = format_info(t->n, ms, visits, root.eval_tag, root.eval.ply, pv.data(), len < (int)pv.size() ? len : (int)pv.size(), line)))
        return rc;
    if (t->sink) {
        if (t->sink(t->sink_user, line.c_str())) *stop = true;
    } else {
        out += line + "\n";
    }
    return TZ_OK;
}

// main.rs:216-296
int on_go(tz_tei* t, const Parsed& p, std::string& out) {
    using clock = std::chrono::steady_clock;
    int rc;
    tz_state pos;
    tz_root_info root;
    if ((rc = tz_search_get_positions(t->s, &pos))) return rc;
    if ((rc = tz_search_root_info(t->s, &root))) return rc;
    auto no_moves = [&]() {
        out += "info string error: the position has no moves to search\n";
        return tz_fail(TZ_ESTATE, "tz_tei_line: go on a root without children");
    };
    if (root.is_terminal_env) return no_moves();  // the game is over: no round would ever give the root a child
    const int64_t mask = p.numbers[0];
    auto given = [&](int opt) { return (mask >> opt & 1) != 0; };
    const bool white = pos.to_move == 0;
    bool have_nodes = false, have_move_time = false, have_time = false, have_inc = false;
    uint64_t nodes = 0, move_time = 0, my_time = 0, my_inc = 0;
    if (given(TZ_TEI_GO_NODES)) have_nodes = true, nodes = (uint64_t)p.numbers[1 + TZ_TEI_GO_NODES];
    if (given(TZ_TEI_GO_INFINITE)) have_nodes = true, nodes = UINT64_MAX;  // main.rs:233
    if (given(TZ_TEI_GO_MOVETIME)) have_move_time = true, move_time = (uint64_t)p.numbers[1 + TZ_TEI_GO_MOVETIME];
    const int time_opt = white ? TZ_TEI_GO_WTIME : TZ_TEI_GO_BTIME, inc_opt = white ? TZ_TEI_GO_WINC : TZ_TEI_GO_BINC;
    if (given(time_opt)) have_time = true, my_time = (uint64_t)p.numbers[1 + time_opt];
    if (given(inc_opt)) have_inc = true, my_inc = (uint64_t)p.numbers[1 + inc_opt];
    if (given(white ? TZ_TEI_GO_BTIME : TZ_TEI_GO_WTIME) || given(white ? TZ_TEI_GO_BINC : TZ_TEI_GO_WINC))
        out += "info string warning: ignored `go` options of the side not to move\n";
    if (!have_nodes && !have_move_time && (!have_time || !have_inc)) out += "info string warning: no understood stopping condition given\n";
    if (!have_move_time && have_time && have_inc) {  // very basic time management, main.rs:241-243
        have_move_time = true;
        move_time = my_time / 10 + 3 * my_inc / 4;
    }
    const uint64_t visits_at_start = root.visit_count;
    bool sent_info = false, stop = false;
    const clock::time_point start = clock::now();
    clock::time_point last_info = start;
    auto ms_since = [](clock::time_point a) {
        return (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(clock::now() - a).count();
    };
    for (;;) {
        uint32_t used = 0, cap = 0;
        if ((rc = tz_search_pool_usage(t->s, &used, &cap))) return rc;
        if ((uint64_t)(cap - used) < (uint64_t)t->leaves * (uint64_t)t->max_actions) {
            out += "info string node pool full\n";
            break;
        }
        if ((rc = tz_search_simulate_batch(t->s, &BETA, t->leaves, 1))) return rc;
        if ((rc = tz_search_root_info(t->s, &root))) return rc;  // synchronises; an error of the round surfaces here
        const uint64_t visits = root.visit_count - visits_at_start;
        const uint64_t elapsed = ms_since(start);
        const bool done = (have_nodes && visits >= nodes) || (have_move_time && elapsed >= move_time);
        if (ms_since(last_info) >= (uint64_t)t->info_interval_ms) {
            if ((rc = emit_info(t, elapsed, visits, root, out, &stop))) return rc;
            sent_info = true;
            last_info = clock::now();
        }
        if (done || stop || t->stops_announced.load(std::memory_order_acquire) > t->stop_lines) break;
    }
    if (root.n_children == 0) return no_moves();
    if (!sent_info && (rc = emit_info(t, ms_since(start), root.visit_count - visits_at_start, root, out, &stop))) return rc;
    uint16_t best = 0xFFFF;
    if ((rc = tz_search_select_best_actions(t->s, &best))) return rc;
    out += "bestmove " + ptn(t, best) + "\n";
    return TZ_OK;
}

}  // namespace

int tz_tei_create(tz_search* one_tree, int leaves, tz_tei** out) {
    if (!one_tree || !out || leaves < 1) return tz_fail(TZ_EINVAL, "tz_tei_create: bad argument");
    int batch = 0, n = 0, half_komi = 0, max_actions = 0, rc;
    if ((rc = tz_search_shape(one_tree, &batch, &n, &half_komi, &max_actions))) return rc;
    if (batch != 1) return tz_fail(TZ_EINVAL, "tz_tei_create: the engine searches one tree (a handle with a batch of 1)");
    if (leaves > TZ_SIMULATE_BATCH_MAX_SLOTS) return tz_fail(TZ_EINVAL, "tz_tei_create: leaves exceeds TZ_SIMULATE_BATCH_MAX_SLOTS");
    tz_tei* t = new tz_tei;
    t->s = one_tree;
    t->leaves = leaves;
    t->n = n;
    t->half_komi = half_komi;
    t->max_actions = max_actions;
    tz_state st;
    if (!(rc = start_state(t, &st)) && !(rc = reset_to(t, st))) rc = tz_search_simulate(one_tree, &BETA, 1);  // main.rs:139-141
    if (!rc) rc = tz_search_sync(one_tree);
    if (rc) {
        delete t;
        return rc;
    }
    t->have_last = true;  // Position::StartPos with no moves, main.rs:154-155
    *out = t;
    return TZ_OK;
}

int tz_tei_destroy(tz_tei* t) {
    delete t;
    return TZ_OK;
}

int tz_tei_stop(tz_tei* t) {
    if (!t) return TZ_EINVAL;  // no tz_fail: the error text belongs to the thread inside tz_tei_line
    t->stops_announced.fetch_add(1, std::memory_order_release);
    return TZ_OK;
}

int tz_tei_set_sink(tz_tei* t, int (*sink)(void*, const char*), void* user) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_tei_set_sink: null handle");
    t->sink = sink;
    t->sink_user = user;
    return TZ_OK;
}

int tz_tei_set_info_interval(tz_tei* t, int ms) {
    if (!t || ms < 0) return tz_fail(TZ_EINVAL, "tz_tei_set_info_interval: bad argument");
    t->info_interval_ms = ms;
    return TZ_OK;
}

int tz_tei_line(tz_tei* t, const char* line, char* out, uint64_t cap, uint64_t* size_out, int* quit_out) {
    if (!t || !line || !size_out || !quit_out || (cap && !out)) return tz_fail(TZ_EINVAL, "tz_tei_line: bad argument");
    *quit_out = 0;
    std::string o;
    Parsed p;
    int rc = parse_line(line, t->n, p);
    if (rc) {
        o = "info string error: parse error: " + p.err_text + "\n";
        tz_set_error("tz_tei_line: parse error: " + p.err_text);
    } else {
        switch (p.kind) {
            case TZ_TEI_ISREADY: o = "readyok\n"; break;
            case TZ_TEI_TEI: o = "info string warning: tei does not make sense here\n"; break;
            case TZ_TEI_SETOPTION: o = "info string warning: it's too late to specify options\n"; break;
            case TZ_TEI_NEWGAME:
                if (p.numbers[0] != t->n) {  // main.rs:167-170 leaves the main loop
                    o = "info string error: the engine is built only for size " + std::to_string(t->n) + "\n";
                    *quit_out = 1;
                    rc = tz_fail(TZ_EINVAL, "tz_tei_line: teinewgame with another board size");
                } else {
                    tz_state st;
                    if (!(rc = start_state(t, &st))) rc = reset_to(t, st);
                    t->have_last = false;  // the reference keeps last_position / last_moves over a new game
                    t->last_moves.clear();
                }
                break;
            case TZ_TEI_POSITION: rc = on_position(t, p, o); break;
            case TZ_TEI_GO: rc = on_go(t, p, o); break;
            case TZ_TEI_STOP: t->stop_lines++; break;
            case TZ_TEI_QUIT:
                t->stop_lines++;
                *quit_out = 1;
                break;
        }
    }
    *size_out = o.size();
    if (cap) {
        const size_t k = o.size() < cap - 1 ? o.size() : (size_t)(cap - 1);
        memcpy(out, o.data(), k);
        out[k] = 0;
    }
    return rc;
}

int tz_tei_parse(const char* line, int n, int* kind_out, int64_t* numbers_out, uint16_t* moves_out, int moves_cap, int* n_moves_out,
                 char* tps_out, int tps_cap) {
    if (!line || n < 3 || n > 6 || !kind_out || !numbers_out || !n_moves_out || moves_cap < 0 || (moves_cap && !moves_out) ||
        tps_cap < 0 || (tps_cap && !tps_out))
        return tz_fail(TZ_EINVAL, "tz_tei_parse: bad argument");
    Parsed p;
    const int rc = parse_line(line, n, p);
    *kind_out = p.kind;
    memcpy(numbers_out, p.numbers, sizeof p.numbers);
    *n_moves_out = (int)p.moves.size();
    if (tps_cap) tps_out[0] = 0;
    if (rc) return tz_fail(rc, "parse error: " + p.err_text);
    if ((int)p.moves.size() > moves_cap) return tz_fail(TZ_EINVAL, "tz_tei_parse: more moves than moves_cap");
    if (!p.moves.empty()) memcpy(moves_out, p.moves.data(), p.moves.size() * sizeof(uint16_t));
    if (!p.text.empty()) {
        if ((int)p.text.size() + 1 > tps_cap) return tz_fail(TZ_EINVAL, "tz_tei_parse: tps_cap too small");
        memcpy(tps_out, p.text.c_str(), p.text.size() + 1);
    }
    return TZ_OK;
}

int tz_tei_format_info(int n, uint64_t time_ms, uint64_t nodes, uint8_t eval_tag, uint32_t eval_bits, const uint16_t* pv, int pv_len,
                       char* out, int cap) {
    if (n < 3 || n > 6 || pv_len < 0 || (pv_len && !pv) || !out || cap <= 0 || eval_tag > TZ_EVAL_DRAW)
        return tz_fail(TZ_EINVAL, "tz_tei_format_info: bad argument");
    std::string o;
    const int rc = format_info(n, time_ms, nodes, eval_tag, eval_bits, pv, pv_len, o);
    if (rc) return rc;
    if ((int)o.size() + 1 > cap) return tz_fail(TZ_EINVAL, "tz_tei_format_info: buffer too small");
    memcpy(out, o.c_str(), o.size() + 1);
    return (int)o.size();
}
