// tests/simulate_batch_ref.cpp — CPU restatement of Node::simulate_batch (takzero/src/search/node/mcts.rs:268-328) and
// Node::principal_variation (node/mod.rs:40-62, 87-90) for the tests of tz_search_simulate_batch / tz_search_principal_variation.
//
// TEST INFRASTRUCTURE ONLY.  Everything that computes is the oracle's (oracle/mcts.hpp): Node<TakEnv>::forward,
// backward_known_eval, backward_network_eval, select_best_action, descend and softmax, which the reference's known answers pin
// (tests/test_oracle_kat.py).  This file only adds the loop around them, in the reference's order, and counts the events a test
// case is there for.  Built by tests/simulate_batch_util.py with the flags of oracle/Makefile.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../oracle/mcts.hpp"
#include "../oracle/tak.hpp"

using namespace tzo;

extern "C" {

// the AGENT_FN of tests/oracle_lib.py: logits_out is [n_envs][amax]
typedef void (*sbr_agent_fn)(void* user, int n_envs, const tz_state* states, const uint16_t* legal_idx, const int32_t* legal_count,
                             int amax, float* logits_out, float* value_out, float* variance_out);
}

namespace {

struct CallbackAgent : Agent<TakEnv> {
    sbr_agent_fn fn = nullptr;
    void* user = nullptr;
    void policy_value_uncertainty(const std::vector<TakEnv>& envs, const std::vector<std::vector<int>>& actions,
                                  std::vector<std::vector<float>>& logits, std::vector<float>& value,
                                  std::vector<float>& variance) override {
        const int b = (int)envs.size();
        int amax = 1;
        for (auto& a : actions) amax = std::max(amax, (int)a.size());
        std::vector<tz_state> st(b);
        std::vector<uint16_t> idx((size_t)b * amax, 0);
        std::vector<int32_t> cnt(b);
        for (int i = 0; i < b; i++) {
            envs[i].g.to_state(st[i]);
            cnt[i] = (int)actions[i].size();
            for (size_t j = 0; j < actions[i].size(); j++) idx[(size_t)i * amax + j] = (uint16_t)actions[i][j];
        }
        std::vector<float> lo((size_t)b * amax, 0.0f);
        value.assign(b, 0.0f);
        variance.assign(b, 0.0f);
        fn(user, b, st.data(), idx.data(), cnt.data(), amax, lo.data(), value.data(), variance.data());
        logits.clear();
        for (int i = 0; i < b; i++) logits.emplace_back(lo.begin() + (size_t)i * amax, lo.begin() + (size_t)i * amax + cnt[i]);
    }
};

enum { FORWARDS, KNOWN_IN_ROUND, LEAVES, DUPLICATE_LEAVES, SHORT_ROUNDS, N_COUNTS };

struct Search {
    int n = 0, half_komi = 0;
    std::vector<Node<TakEnv>> nodes;
    std::vector<TakEnv> envs;
    std::unique_ptr<Agent<TakEnv>> agent;
    uint64_t counts[N_COUNTS] = {0, 0, 0, 0, 0};
    std::vector<uint32_t> round_leaves;  // per tree: the leaves it collected in its latest simulate_batch round
};

// mcts.rs:268-328, line for line
void simulate_batch(Search& s, size_t game, float beta, size_t batch_size) {
    Node<TakEnv>& root = s.nodes[game];
    const TakEnv& env = s.envs[game];
    std::vector<std::vector<size_t>> trajectories;
    std::vector<std::vector<int>> actionss;
    std::vector<TakEnv> envs;
    for (size_t i = 0; i < batch_size * 4; i++) {                       // :281
        std::vector<size_t> trajectory;
        TakEnv e = env;                                                // env.clone()
        Eval known;
        s.counts[FORWARDS]++;
        if (root.forward(trajectory, e, beta, known) == Node<TakEnv>::KNOWN) {
            root.backward_known_eval(trajectory, 0, known);            // :284
            s.counts[KNOWN_IN_ROUND]++;
        } else {
            if (std::find(trajectories.begin(), trajectories.end(), trajectory) != trajectories.end()) s.counts[DUPLICATE_LEAVES]++;
            trajectories.push_back(trajectory);
            std::vector<int> actions;
            e.populate_actions(actions);
            actionss.push_back(std::move(actions));
            envs.push_back(e);
        }
        if (trajectories.size() == batch_size) break;                   // :297
    }
    s.counts[LEAVES] += trajectories.size();
    s.round_leaves[game] = (uint32_t)trajectories.size();
    if (trajectories.size() < batch_size) s.counts[SHORT_ROUNDS]++;
    if (trajectories.empty()) return;                                   // :303
    std::vector<std::vector<float>> logits;
    std::vector<float> value, variance, probs;
    s.agent->policy_value_uncertainty(envs, actionss, logits, value, variance);
    for (size_t i = 0; i < trajectories.size(); i++) {                  // :307-327
        softmax(logits[i], probs);
        root.backward_network_eval(trajectories[i], 0, actionss[i], logits[i], probs, value[i], variance[i]);
    }
}

const Node<TakEnv>* walk(const Search& s, int game, const uint16_t* path, int path_len) {
    const Node<TakEnv>* node = &s.nodes[game];
    for (int d = 0; d < path_len; d++) {
        const Node<TakEnv>* next = nullptr;
        for (auto& c : node->children)
            if (c.first == (int)path[d]) {
                next = &c.second;
                break;
            }
        if (!next) return nullptr;
        node = next;
    }
    return node;
}

}  // namespace

extern "C" {

Search* sbr_create(int agent_kind, sbr_agent_fn fn, void* user, int batch, int n, int half_komi) {
    Search* s = new Search();
    s->n = n;
    s->half_komi = half_komi;
    s->nodes.resize(batch);
    s->envs.resize(batch);
    s->round_leaves.assign(batch, 0);
    for (auto& e : s->envs) e.g = Game(n, half_komi);
    if (agent_kind == TZ_AGENT_DUMMY) s->agent.reset(new DummyAgent<TakEnv>());
    else if (agent_kind == TZ_AGENT_SIMPLE) s->agent.reset(new SimpleAgent());
    else {
        auto* c = new CallbackAgent();
        c->fn = fn;
        c->user = user;
        s->agent.reset(c);
    }
    return s;
}
void sbr_destroy(Search* s) { delete s; }

int sbr_set_positions(Search* s, int count, const int32_t* game_idx, const tz_state* states) {
    for (int i = 0; i < count; i++) {
        const int g = game_idx[i];
        if (g < 0 || g >= (int)s->nodes.size()) return -1;
        s->envs[g].g = Game::from_state(states[i]);
        s->nodes[g] = Node<TakEnv>();
    }
    return 0;
}
int sbr_new_openings(Search* s, const int32_t* choice) {
    for (size_t g = 0; g < s->nodes.size(); g++) {
        s->envs[g].g = new_opening(s->n, s->half_komi, choice[g]);
        s->nodes[g] = Node<TakEnv>();
    }
    return 0;
}

// Node::simulate_batch on every root, `rounds` times: trees are independent, so the order of the two loops does not matter
int sbr_simulate_batch(Search* s, const float* betas, int leaves, int rounds) {
    if (leaves < 1 || rounds < 0) return -1;
    for (int r = 0; r < rounds; r++)
        for (size_t g = 0; g < s->nodes.size(); g++) simulate_batch(*s, g, betas[g], (size_t)leaves);
    return 0;
}

// BatchedMCTS::simulate (batched.rs:63-128), `n_sims` times: one forward per tree, one agent call for the leaves of all trees, in
// tree order, then the backward passes.  A forward counts as a forward and a leaf as a leaf, as the device's counters count them.
int sbr_simulate(Search* s, const float* betas, int n_sims) {
    if (n_sims < 0) return -1;
    for (int r = 0; r < n_sims; r++) {
        std::vector<size_t> games;
        std::vector<std::vector<size_t>> trajectories;
        std::vector<std::vector<int>> actionss;
        std::vector<TakEnv> envs;
        for (size_t g = 0; g < s->nodes.size(); g++) {
            std::vector<size_t> trajectory;
            TakEnv e = s->envs[g];
            Eval known;
            s->counts[FORWARDS]++;
            if (s->nodes[g].forward(trajectory, e, betas[g], known) == Node<TakEnv>::KNOWN) {
                s->nodes[g].backward_known_eval(trajectory, 0, known);
                continue;
            }
            std::vector<int> actions;
            e.populate_actions(actions);
            games.push_back(g);
            trajectories.push_back(std::move(trajectory));
            actionss.push_back(std::move(actions));
            envs.push_back(e);
        }
        s->counts[LEAVES] += games.size();
        if (games.empty()) continue;
        std::vector<std::vector<float>> logits;
        std::vector<float> value, variance, probs;
        s->agent->policy_value_uncertainty(envs, actionss, logits, value, variance);
        for (size_t i = 0; i < games.size(); i++) {
            softmax(logits[i], probs);
            s->nodes[games[i]].backward_network_eval(trajectories[i], 0, actionss[i], logits[i], probs, value[i], variance[i]);
        }
    }
    return 0;
}

// BatchedMCTS::step (batched.rs:131-144): descend + env.step, skipped for terminal roots
int sbr_step(Search* s, const uint16_t* actions) {
    for (size_t g = 0; g < s->nodes.size(); g++) {
        if (s->nodes[g].is_terminal()) continue;
        s->nodes[g].descend(actions[g]);
        s->envs[g].step(actions[g]);
    }
    return 0;
}

// per-call event counts since creation: forwards made, Known results inside a round, leaves collected, leaves already collected
// earlier in the same round, (tree, round) pairs that ended short of `leaves`
void sbr_counts(Search* s, uint64_t* out) { memcpy(out, s->counts, sizeof s->counts); }
// per tree, the leaves collected in the latest simulate_batch round: what the device's offset[] and index[] are built from
void sbr_round_leaves(Search* s, uint32_t* out) { memcpy(out, s->round_leaves.data(), s->round_leaves.size() * sizeof(uint32_t)); }

static size_t tree_size(const Node<TakEnv>& node) {
    size_t n = 1;
    for (auto& c : node.children) n += tree_size(c.second);
    return n;
}
// nodes of one tree, the root included: the slots the same tree takes in a node pool of the device
uint64_t sbr_tree_size(Search* s, int game) { return tree_size(s->nodes[game]); }

// Node::principal_variation: returns the full length, writes at most cap moves
int sbr_principal_variation(Search* s, int game, uint16_t* moves_out, int cap) {
    const Node<TakEnv>* node = &s->nodes[game];
    int len = 0;
    while (!(node->needs_initialization() || node->is_terminal())) {
        const int best = node->select_best_action();
        const Node<TakEnv>* next = nullptr;
        for (auto& c : node->children)
            if (c.first == best) {
                next = &c.second;
                break;
            }
        if (!next) return -1;  // "Best action not found among node's children"
        if (len < cap) moves_out[len] = (uint16_t)best;
        len++;
        node = next;
    }
    return len;
}

// the node query of tzo_search_node (oracle/capi.cpp)
int sbr_node(Search* s, int game, const uint16_t* path, int path_len, tz_root_info* node_out, int amax, uint16_t* move_idx,
             uint32_t* visits, uint8_t* eval_tag, uint32_t* eval_bits, float* logit, float* prob, float* std_dev) {
    const Node<TakEnv>* node = walk(*s, game, path, path_len);
    if (!node) return -1;
    if ((int)node->children.size() > amax) return -1;
    if (node_out) {
        memset(node_out, 0, sizeof *node_out);
        node_out->visit_count = node->visit_count;
        node_out->n_children = (uint32_t)node->children.size();
        node_out->eval_tag = node->evaluation.tag;
        node_out->eval.ply = node->evaluation.bits();
        node_out->std_dev = node->std_dev;
        node_out->logit = node->logit;
        node_out->probability = node->probability;
        node_out->ply = (uint16_t)(s->envs[game].steps() + path_len);
        node_out->is_terminal_env = node->is_terminal();
    }
    for (size_t i = 0; i < node->children.size(); i++) {
        const Node<TakEnv>& c = node->children[i].second;
        if (move_idx) move_idx[i] = (uint16_t)node->children[i].first;
        if (visits) visits[i] = c.visit_count;
        if (eval_tag) eval_tag[i] = c.evaluation.tag;
        if (eval_bits) eval_bits[i] = c.evaluation.bits();
        if (logit) logit[i] = c.logit;
        if (prob) prob[i] = c.probability;
        if (std_dev) std_dev[i] = c.std_dev;
    }
    return 0;
}

}  // extern "C"
