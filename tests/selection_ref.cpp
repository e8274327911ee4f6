// tests/selection_ref.cpp — CPU restatement of the three in-tree selection rules of takzero/src/search/node/policy.rs
// (select_with_puct :78-95, select_with_uct :104-117, select_with_improved_policy :57-69) and of Node::forward (mcts.rs:107-138)
// with the rule as an argument, for the tests of tz_search_set_selection.
//
// TEST INFRASTRUCTURE ONLY.  What is restated here: the three select_with_* functions, forward, and the loops that call forward
// (BatchedMCTS::simulate, Node::simulate_batch, and the forward / backward body of gumbel_sequential_halving), with the loop
// structure of oracle/mcts.hpp.  Everything else that computes is the oracle's own, unchanged: backward_known_eval,
// backward_network_eval, improved_policy, softmax, Eval and the rules of Tak.  tests/test_selection_ref.py pins the restatement:
// with rule PUCT it must give the oracle's trees.  Built by tests/selection_util.py with the flags of oracle/Makefile.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../oracle/mcts.hpp"
#include "../oracle/tak.hpp"

using namespace tzo;

extern "C" {
// the AGENT_FN of tests/oracle_lib.py: logits_out is [n_envs][amax]
typedef void (*sel_agent_fn)(void* user, int n_envs, const tz_state* states, const uint16_t* legal_idx, const int32_t* legal_count,
                             int amax, float* logits_out, float* value_out, float* variance_out);
}

namespace {

enum { RULE_PUCT = 0, RULE_UCT = 1, RULE_IMPROVED = 2 };
typedef Node<TakEnv> TNode;

struct CallbackAgent : Agent<TakEnv> {
    sel_agent_fn fn = nullptr;
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

struct Search {
    int n = 0, half_komi = 0, rule = RULE_PUCT;
    bool nan_seen = false;  // a NaN score: the reference's NotNan panics (policy.rs:113)
    std::vector<TNode> nodes;
    std::vector<TakEnv> envs;
    std::unique_ptr<Agent<TakEnv>> agent;
};

// the filter all three rules share, policy.rs:62 / :83 / :109
inline bool eligible(const TNode& parent, const TNode& child) { return parent.evaluation.is_loss() || !child.evaluation.is_win(); }

// Iterator::max_by_key over (index, score): the last maximum
struct LastMax {
    bool have = false;
    size_t best = 0;
    float best_score = 0.0f;
    void offer(size_t i, float score) {
        if (!have || !(score < best_score)) {
            have = true;
            best = i;
            best_score = score;
        }
    }
};

// policy.rs:78-95
size_t select_with_puct(const TNode& node, float beta) {
    const float parent = (float)node.visit_count;
    LastMax m;
    for (size_t i = 0; i < node.children.size(); i++) {
        const TNode& ch = node.children[i].second;
        if (!eligible(node, ch)) continue;
        const float q = ch.q_value();
        const float puct = ucb_with_predictor(parent, (float)ch.visit_count, ch.probability);
        m.offer(i, (q + puct) + ch.std_dev * beta);
    }
    return m.best;
}

// policy.rs:158-164
inline float upper_confidence_bound(float parent_visit_count, float visit_count) {
    return 1.0f * sqrtf(m_ln(parent_visit_count) / visit_count);
}

// policy.rs:104-117
size_t select_with_uct(const TNode& node, float beta, bool& nan) {
    const float parent = (float)node.visit_count;
    LastMax m;
    for (size_t i = 0; i < node.children.size(); i++) {
        const TNode& ch = node.children[i].second;
        if (!eligible(node, ch)) continue;
        const float q = ch.q_value();
        const float uct = upper_confidence_bound(parent, (float)ch.visit_count);
        const float score = (q + uct) + ch.std_dev * beta;
        nan = nan || !(score == score);
        m.offer(i, score);
    }
    return m.best;
}

// policy.rs:57-69; improved_policy (:36-48) and most_visited_count (:23-29) are the oracle's
size_t select_with_improved_policy(const TNode& node, bool& nan) {
    std::vector<float> pi;
    node.improved_policy((float)node.most_visited_count(), pi);
    LastMax m;
    for (size_t i = 0; i < node.children.size(); i++) {
        const TNode& ch = node.children[i].second;
        if (!eligible(node, ch)) continue;
        const float score = pi[i] - (float)ch.visit_count / (float)(node.visit_count + 1u);
        nan = nan || !(score == score);
        m.offer(i, score);
    }
    return m.best;
}

size_t select(const TNode& node, int rule, float beta, bool& nan) {
    return rule == RULE_UCT ? select_with_uct(node, beta, nan) : rule == RULE_IMPROVED ? select_with_improved_policy(node, nan)
                                                                                       : select_with_puct(node, beta);
}

// mcts.rs:107-138 with the rule of :132 as an argument
TNode::ForwardKind forward(Search& s, TNode& root, std::vector<size_t>& trajectory, TakEnv& env, float beta, Eval& known_out) {
    TNode* node = &root;
    for (;;) {
        node->visit_count += 1;
        if (node->is_terminal()) {
            known_out = node->evaluation;
            return TNode::KNOWN;
        }
        if (node->needs_initialization()) {
            const int t = env.terminal();
            if (t != TZ_TERMINAL_NONE) {
                node->evaluation = eval_from_terminal(t);
                node->std_dev = 0.0f;
                known_out = node->evaluation;
                return TNode::KNOWN;
            }
            return TNode::NEEDS_NETWORK;
        }
        const size_t index = select(*node, s.rule, beta, s.nan_seen);
        trajectory.push_back(index);
        env.step(node->children[index].first);
        node = &node->children[index].second;
    }
}

// BatchedMCTS::simulate_from of oracle/mcts.hpp (batched.rs:63-128 and the inner loop of :265-335)
void simulate_from(Search& s, std::vector<TNode*>& roots, const std::vector<TakEnv>& root_envs, const float* betas) {
    struct Pending {
        TNode* node;
        std::vector<size_t> traj;
    };
    std::vector<Pending> pend;
    std::vector<TakEnv> env_batch;
    std::vector<std::vector<int>> act_batch;
    for (size_t g = 0; g < roots.size(); g++) {
        std::vector<size_t> traj;
        TakEnv env = root_envs[g];
        Eval known;
        if (forward(s, *roots[g], traj, env, betas[g], known) == TNode::KNOWN) {
            roots[g]->backward_known_eval(traj, 0, known);
        } else {
            std::vector<int> acts;
            env.populate_actions(acts);
            env_batch.push_back(env);
            act_batch.push_back(std::move(acts));
            pend.push_back({roots[g], std::move(traj)});
        }
    }
    if (env_batch.empty()) return;
    std::vector<std::vector<float>> logits;
    std::vector<float> value, variance, probs;
    s.agent->policy_value_uncertainty(env_batch, act_batch, logits, value, variance);
    for (size_t i = 0; i < pend.size(); i++) {
        softmax(logits[i], probs);
        pend[i].node->backward_network_eval(pend[i].traj, 0, act_batch[i], logits[i], probs, value[i], variance[i]);
    }
}

void simulate(Search& s, const float* betas) {
    std::vector<TNode*> roots(s.nodes.size());
    for (size_t g = 0; g < s.nodes.size(); g++) roots[g] = &s.nodes[g];
    simulate_from(s, roots, s.envs, betas);
}

// mcts.rs:268-328 as in tests/simulate_batch_ref.cpp
void simulate_batch(Search& s, TNode& root, const TakEnv& env, float beta, size_t batch_size) {
    std::vector<std::vector<size_t>> trajectories;
    std::vector<std::vector<int>> actionss;
    std::vector<TakEnv> envs;
    for (size_t i = 0; i < batch_size * 4; i++) {
        std::vector<size_t> trajectory;
        TakEnv e = env;
        Eval known;
        if (forward(s, root, trajectory, e, beta, known) == TNode::KNOWN) {
            root.backward_known_eval(trajectory, 0, known);
        } else {
            trajectories.push_back(trajectory);
            std::vector<int> actions;
            e.populate_actions(actions);
            actionss.push_back(std::move(actions));
            envs.push_back(e);
        }
        if (trajectories.size() == batch_size) break;
    }
    if (trajectories.empty()) return;
    std::vector<std::vector<float>> logits;
    std::vector<float> value, variance, probs;
    s.agent->policy_value_uncertainty(envs, actionss, logits, value, variance);
    for (size_t i = 0; i < trajectories.size(); i++) {
        softmax(logits[i], probs);
        root.backward_network_eval(trajectories[i], 0, actionss[i], logits[i], probs, value[i], variance[i]);
    }
}

// BatchedMCTS::gumbel_sequential_halving of oracle/mcts.hpp (batched.rs:207-409); gumbel is [batch][amax]
void gumbel_sequential_halving(Search& s, const float* betas, size_t sampled_actions, uint32_t search_budget, const float* gumbel,
                               int amax, uint16_t* selected) {
    const size_t batch = s.nodes.size();
    const uint32_t lg = 31 - __builtin_clz((unsigned)sampled_actions);
    simulate(s, betas);
    struct Cand {
        float key;
        size_t child;
    };
    std::vector<std::vector<Cand>> sets(batch);
    for (size_t g = 0; g < batch; g++) {
        auto& set = sets[g];
        for (size_t i = 0; i < s.nodes[g].children.size(); i++)
            set.push_back({s.nodes[g].children[i].second.logit + gumbel[g * (size_t)amax + i], i});
        std::stable_sort(set.begin(), set.end(), [](const Cand& a, const Cand& b) { return a.key > b.key; });
        if (set.size() > sampled_actions) set.resize(sampled_actions);
    }
    uint32_t steps = lg, visits_per_step = search_budget / steps, visits_to_most = 0;
    size_t remaining = sampled_actions;
    std::vector<float> zero_betas(batch, 0.0f);
    for (uint32_t st = 0; st < steps; st++) {
        const uint32_t visits_per_action = visits_per_step / (uint32_t)remaining;
        for (size_t i = 0; i < remaining; i++) {
            std::vector<TNode*> roots(batch);
            std::vector<TakEnv> cenvs;
            cenvs.reserve(batch);
            for (size_t g = 0; g < batch; g++) {
                const size_t k = i % sets[g].size();
                auto& ch = s.nodes[g].children[sets[g][k].child];
                TakEnv env = s.envs[g];
                env.step(ch.first);
                roots[g] = &ch.second;
                cenvs.push_back(env);
            }
            for (uint32_t v = 0; v < visits_per_action; v++) simulate_from(s, roots, cenvs, zero_betas.data());
        }
        visits_to_most += visits_per_action;
        remaining /= 2;
        for (size_t g = 0; g < batch; g++) {
            auto& set = sets[g];
            const float beta = betas[g];
            std::vector<std::pair<float, Cand>> keyed;
            for (auto& c : set) {
                const TNode& ch = s.nodes[g].children[c.child].second;
                const float k = c.key + sigma_select(ch.evaluation.negate().to_notnan(), ch.std_dev, beta, (float)visits_to_most);
                keyed.push_back({k, c});
            }
            std::stable_sort(keyed.begin(), keyed.end(),
                             [](const std::pair<float, Cand>& a, const std::pair<float, Cand>& b) { return a.first > b.first; });
            set.clear();
            for (size_t j = 0; j < keyed.size() && j < remaining; j++) set.push_back(keyed[j].second);
        }
    }
    for (size_t g = 0; g < batch; g++) selected[g] = (uint16_t)s.nodes[g].children[sets[g][0].child].first;
    for (auto& node : s.nodes) {  // batched.rs:373-406
        uint32_t sum = 0;
        bool any_loss = false, all_known = true;
        for (auto& c : node.children) {
            sum += c.second.visit_count;
            any_loss = any_loss || c.second.evaluation.is_loss();
            all_known = all_known && c.second.evaluation.is_known();
        }
        node.visit_count = sum + 1;
        if (any_loss || all_known) {
            node.evaluation = node.min_child_eval().negate();
            node.std_dev = 0.0f;
        } else {
            float sp = 0.0f, wq = 0.0f;
            for (auto& c : node.children)
                if (c.second.visit_count > 0) sp = sp + c.second.probability;
            for (auto& c : node.children)
                if (c.second.visit_count > 0) wq = wq + c.second.probability * c.second.evaluation.negate().to_f32();
            node.evaluation = Eval::Value(wq / sp);
        }
    }
}

const TNode* walk(const Search& s, int game, const uint16_t* path, int path_len) {
    const TNode* node = &s.nodes[game];
    for (int d = 0; d < path_len; d++) {
        const TNode* next = nullptr;
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

float sel_m_ln(float x) { return m_ln(x); }

Search* sel_create(int agent_kind, sel_agent_fn fn, void* user, int batch, int n, int half_komi) {
    Search* s = new Search();
    s->n = n;
    s->half_komi = half_komi;
    s->nodes.resize(batch);
    s->envs.resize(batch);
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
void sel_destroy(Search* s) { delete s; }

int sel_set_rule(Search* s, int rule) {
    if (rule < RULE_PUCT || rule > RULE_IMPROVED) return -1;
    s->rule = rule;
    return 0;
}
int sel_nan_seen(Search* s) { return s->nan_seen ? 1 : 0; }

int sel_set_positions(Search* s, int count, const int32_t* game_idx, const tz_state* states) {
    for (int i = 0; i < count; i++) {
        const int g = game_idx[i];
        if (g < 0 || g >= (int)s->nodes.size()) return -1;
        s->envs[g].g = Game::from_state(states[i]);
        s->nodes[g] = TNode();
    }
    return 0;
}
int sel_new_openings(Search* s, const int32_t* choice) {
    for (size_t g = 0; g < s->nodes.size(); g++) {
        s->envs[g].g = new_opening(s->n, s->half_komi, choice[g]);
        s->nodes[g] = TNode();
    }
    return 0;
}

int sel_simulate(Search* s, const float* betas, int n_sims) {
    for (int i = 0; i < n_sims; i++) simulate(*s, betas);
    return 0;
}
int sel_simulate_batch(Search* s, const float* betas, int leaves, int rounds) {
    if (leaves < 1 || rounds < 0) return -1;
    for (int r = 0; r < rounds; r++)
        for (size_t g = 0; g < s->nodes.size(); g++) simulate_batch(*s, s->nodes[g], s->envs[g], betas[g], (size_t)leaves);
    return 0;
}
int sel_gumbel_sh(Search* s, const float* betas, int sampled_actions, int search_budget, const float* gumbel, int amax,
                  uint16_t* selected) {
    gumbel_sequential_halving(*s, betas, (size_t)sampled_actions, (uint32_t)search_budget, gumbel, amax, selected);
    return 0;
}

// the child index `rule` picks at game's root in a forward that has just incremented the root's visit count
int sel_select_at_root(Search* s, int game, int rule, float beta) {
    TNode& node = s->nodes[game];
    if (node.children.empty()) return -1;
    bool nan = false;
    node.visit_count += 1;
    const size_t i = select(node, rule, beta, nan);
    node.visit_count -= 1;
    return nan ? -2 : (int)i;
}

static size_t tree_size(const TNode& node) {
    size_t n = 1;
    for (auto& c : node.children) n += tree_size(c.second);
    return n;
}
// nodes of one tree, the root included: the slots the same tree takes in a node pool of the device
uint64_t sel_tree_size(Search* s, int game) { return tree_size(s->nodes[game]); }

// the node query of tzo_search_node (oracle/capi.cpp)
int sel_node(Search* s, int game, const uint16_t* path, int path_len, tz_root_info* node_out, int amax, uint16_t* move_idx,
             uint32_t* visits, uint8_t* eval_tag, uint32_t* eval_bits, float* logit, float* prob, float* std_dev) {
    const TNode* node = walk(*s, game, path, path_len);
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
        const TNode& c = node->children[i].second;
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
