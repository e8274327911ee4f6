// tz_tree.hip — batched MCTS on the device: one wavefront per game.
//
// Replaces, for B concurrent games stepped in lock-step (takzero/src/search/node/batched.rs:63-128):
//   Node::forward            mcts.rs:107-138   -> descend_kernel   (select with PUCT policy.rs:78-95, UCT :104-117 or the
//                                                  improved policy :57-69, by SearchDev::select_rule)
//   Node::backward_known_eval mcts.rs:141-163  -> descend_kernel   (immediately, as batched.rs:78-82)
//   softmax + backward_network_eval policy.rs:10-19, mcts.rs:171-225 -> expand_kernel
//   propagate_child_eval / node_solver mcts.rs:49-102 -> backup()
//   apply_dirichlet noise.rs:10-26, descend node/mod.rs:95-102, select_best_action node/mod.rs:132-161,
//   step / restart_terminal_envs batched.rs:131-203.
//
// Arithmetic is f32 in exactly the reference's expression order; this file is compiled with
// -ffp-contract=off and uses tz_math.h for exp/ln/powi so results are bit-identical with the
// CPU oracle.  Node statistics are SoA slabs in HBM (tz_engine.h); a node's children are
// contiguous so a child scan is a handful of coalesced loads, and argmax / min / all-known are
// wavefront reductions.
#include "tz_engine.h"
#include "tz_math.h"
#include "tz_tak_dev.h"

using namespace tzd;

namespace {

struct Ev {
    uint32_t tag, bits;
};
__device__ __forceinline__ Ev ev_value(float v) { return Ev{TZ_EVAL_VALUE, tz_float_to_bits(v)}; }
__device__ __forceinline__ bool ev_known(Ev e) { return e.tag != TZ_EVAL_VALUE; }
// eval.rs:40-47
__device__ __forceinline__ Ev ev_negate(Ev e) {
    switch (e.tag) {
        case TZ_EVAL_VALUE: return ev_value(-tz_bits_to_float(e.bits));
        case TZ_EVAL_WIN: return Ev{TZ_EVAL_LOSS, e.bits + 1};
        case TZ_EVAL_DRAW: return Ev{TZ_EVAL_DRAW, e.bits + 1};
        default: return Ev{TZ_EVAL_WIN, e.bits + 1};
    }
}
// eval.rs:95-105
__device__ __forceinline__ float ev_to_f32(Ev e) {
    const float base = tz_powif(TZ_DISCOUNT, e.tag == TZ_EVAL_VALUE ? 0 : (int)e.bits);
    const float x = e.tag == TZ_EVAL_VALUE ? tz_bits_to_float(e.bits)
                    : e.tag == TZ_EVAL_WIN ? 1.0f
                    : e.tag == TZ_EVAL_LOSS ? -1.0f
                                            : 0.0f;
    return base * x;
}
// eval.rs:107-116
__device__ __forceinline__ float ev_to_notnan(Ev e) {
    return e.tag == TZ_EVAL_VALUE ? tz_bits_to_float(e.bits) : ev_to_f32(e);
}
__device__ __forceinline__ int cmpf(float a, float b) { return a < b ? -1 : a > b ? 1 : 0; }
__device__ __forceinline__ int cmpu(uint32_t a, uint32_t b) { return a < b ? -1 : a > b ? 1 : 0; }
// impl Ord for Eval, eval.rs:138-163 (CONTEMPT = -0.05, eval.rs:128)
__device__ __forceinline__ int ev_cmp(Ev a, Ev b) {
    const float contempt = -0.05f;
    switch (a.tag) {
        case TZ_EVAL_VALUE:
            switch (b.tag) {
                case TZ_EVAL_VALUE: return cmpf(tz_bits_to_float(a.bits), tz_bits_to_float(b.bits));
                case TZ_EVAL_WIN: return -1;
                case TZ_EVAL_DRAW: return cmpf(tz_bits_to_float(a.bits), contempt);
                default: return 1;
            }
        case TZ_EVAL_WIN: return b.tag == TZ_EVAL_WIN ? cmpu(b.bits, a.bits) : 1;
        case TZ_EVAL_DRAW:
            switch (b.tag) {
                case TZ_EVAL_VALUE: return cmpf(contempt, tz_bits_to_float(b.bits));
                case TZ_EVAL_WIN: return -1;
                case TZ_EVAL_DRAW: return cmpu(b.bits, a.bits);
                default: return 1;
            }
        default: return b.tag == TZ_EVAL_LOSS ? cmpu(a.bits, b.bits) : -1;
    }
}

__device__ __forceinline__ size_t slab_base(const SearchDev& s, int bank, int g) {
    return ((size_t)bank * s.batch + g) * (size_t)s.cap;
}

__device__ __forceinline__ void load_state(tz_state* dst, const tz_state* src) {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(src);
    uint32_t* b = reinterpret_cast<uint32_t*>(dst);
    for (int i = lane_id(); i < (int)(sizeof(tz_state) / 4); i += 64) b[i] = a[i];
}

__device__ __forceinline__ void write_default_node(const SearchDev& s, size_t i) {
    s.t.eval_tag[i] = TZ_EVAL_VALUE;
    s.t.eval_bits[i] = 0;
    s.t.visits[i] = 0;
    s.t.prob[i] = 0.0f;
    s.t.logit[i] = 0.0f;
    s.t.std_dev[i] = 0.0f;
    s.t.child0[i] = 0;
    s.t.nchild[i] = 0;
    s.t.action[i] = 0xFFFF;
}

// ---- wave reductions over (key, index) pairs -------------------------------------------------
// first minimum of Eval over children [c0, c0+nc), with one child's value overridden (the path
// child whose fresh value is still in registers).  Also reports whether all are known.
__device__ __forceinline__ void children_min_allknown(const SearchDev& s, size_t base, uint32_t c0, int nc,
                                                      uint32_t patch_node, Ev patch, Ev& min_out, bool& all_known) {
    const int l = lane_id();
    Ev best{0, 0};
    int best_i = 0x7fffffff;
    bool known = true;
    for (int i = l; i < nc; i += 64) {
        const uint32_t node = c0 + i;
        Ev e{s.t.eval_tag[base + node], s.t.eval_bits[base + node]};
        if (node == patch_node) e = patch;
        known = known && ev_known(e);
        // The same source form was miscompiled in select_best_child (see there): with more than 64 children the loop kept the tag
        // and the index of the lane's first child.  Here the compiled loop is right; the solved wide roots of
        // tests/test_gpu_action_capacity.py (a best child beyond the first 64) fail if a compiler does to it what it did there.
        if (best_i == 0x7fffffff || ev_cmp(e, best) < 0) {
            best = e;
            best_i = i;
        }
    }
    all_known = __all(known);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Ev o{(uint32_t)__shfl_xor((int)best.tag, d), (uint32_t)__shfl_xor((int)best.bits, d)};
        const int oi = __shfl_xor(best_i, d);
        if (oi != 0x7fffffff) {
            const int c = best_i == 0x7fffffff ? -1 : ev_cmp(o, best);
            if (c < 0 || (c == 0 && oi < best_i)) {
                best = o;
                best_i = oi;
            }
        }
    }
    min_out = best;
}

// mcts.rs:78-102 applied along the recorded path, leaf side first.  tnode/tvis are in LDS
// (node index and visit_count after this simulation's increment).  `stored` is the evaluation
// now stored in the node below the one being processed.
__device__ void backup(const SearchDev& s, size_t base, const uint32_t* tnode, const uint32_t* tvis, int leaf_level,
                       Ev child_eval, float child_var, Ev stored) {
    for (int lvl = leaf_level - 1; lvl >= 0; lvl--) {
        const uint32_t node = tnode[lvl], below = tnode[lvl + 1];
        Ev ev{s.t.eval_tag[base + node], s.t.eval_bits[base + node]};
        float sd = s.t.std_dev[base + node];
        const uint32_t c0 = s.t.child0[base + node];
        const int nc = s.t.nchild[base + node];
        // node_solver, mcts.rs:66-76
        Ev mn;
        bool all_known;
        children_min_allknown(s, base, c0, nc, below, stored, mn, all_known);
        if (child_eval.tag == TZ_EVAL_LOSS || all_known) {
            ev = ev_negate(mn);
            sd = 0.0f;
        }
        Ev up;
        float up_var;
        if (ev_known(ev)) {
            up = ev;
            up_var = sd * sd;
        } else {
            const float negated = ev_to_notnan(ev_negate(child_eval));
            const float n = (float)tvis[lvl];
            float mean = tz_bits_to_float(ev.bits);
            mean = mean + (-mean + negated) / n;
            ev = ev_value(mean);
            sd = sd + (-sd + sqrtf(child_var)) / n;
            up = ev_value(negated * TZ_DISCOUNT);
            up_var = child_var * TZ_DISCOUNT * TZ_DISCOUNT;
        }
        if (lane_id() == 0) {
            s.t.eval_tag[base + node] = (uint8_t)ev.tag;
            s.t.eval_bits[base + node] = ev.bits;
            s.t.std_dev[base + node] = sd;
        }
        stored = ev;
        child_eval = up;
        child_var = up_var;
    }
}

// ---------------------------------------------------------------------------------------------
// Floats in the LDS row of the IMPROVED pass of forward_walk: one per child at the default max_actions, none for the other rules.
template <int N, int RULE>
struct SelectRow {
    static constexpr int LEN = RULE == TZ_SELECT_IMPROVED ? (N <= 5 ? TZ_MAX_ACTIONS : TZ_MAX_ACTIONS_6) : 0;
};

// ---------------------------------------------------------------------------------------------
// Node::forward, mcts.rs:107-138, from `node` with env at that node's position: the walk shared by descend_kernel (one forward per
// launch) and descend_batch_kernel (a round of forwards per launch).  Records the path in tnode/tvis (LDS), leaves env at the leaf's
// position.  Returns 0 Known (in `known`), 1 NeedsNetwork, 2 error (flag set); depth = nodes on the path.
//
// RULE picks the in-tree selection at compile time (the reference switches it by editing mcts.rs:132): TZ_SELECT_PUCT
// policy.rs:78-95, TZ_SELECT_UCT policy.rs:104-117, TZ_SELECT_IMPROVED policy.rs:57-69.  All three filter with
// `parent.is_loss() || !child.is_win()` and break ties towards the last index (Iterator::max_by_key).  prow is the LDS row of the
// IMPROVED pass (SelectRow<N, RULE>::LEN floats) and nullptr in the other instantiations.
//
// IMPROVED and a full node pool: a leaf that was evaluated but not expanded (expand_kernel, non-strict capacity) has no
// children and no known evaluation, so the completion below treats it as needs_initialization() and gives it the parent's
// evaluation although it has been visited.  The reference's heap trees have no such state.
template <int N, int RULE>
__device__ __forceinline__ int forward_walk(const SearchDev& s, size_t base, tz_state& env, uint32_t* tnode, uint32_t* tvis,
                                            uint32_t node, float beta, int& depth, Ev& known, float* prow) {
    const int l = lane_id();
    for (;;) {
        const uint32_t vis = s.t.visits[base + node] + 1;
        if (l == 0) {
            s.t.visits[base + node] = vis;
            tnode[depth] = node;
            tvis[depth] = vis;
        }
        depth++;
        const Ev ev{s.t.eval_tag[base + node], s.t.eval_bits[base + node]};
        const int nc = s.t.nchild[base + node];
        if (ev_known(ev) && ev.bits == 0) {  // is_terminal, node/mod.rs:106-108
            known = ev;
            return 0;
        }
        if (nc == 0 && !ev_known(ev)) {  // needs_initialization, node/mod.rs:83-85
            const int t = terminal<N>(&env);
            if (t != TZ_TERMINAL_NONE) {
                known = Ev{(uint32_t)(t == TZ_TERMINAL_WIN ? TZ_EVAL_WIN : t == TZ_TERMINAL_LOSS ? TZ_EVAL_LOSS : TZ_EVAL_DRAW), 0};
                if (l == 0) {
                    s.t.eval_tag[base + node] = (uint8_t)known.tag;
                    s.t.eval_bits[base + node] = 0;
                    s.t.std_dev[base + node] = 0.0f;
                }
                return 0;
            }
            return 1;
        }
        if (depth >= TZ_MAX_DEPTH) {
            if (l == 0) atomicMax(s.error_flag, 2);
            return 2;
        }
        // the selection rule (ties -> last index: Iterator::max_by_key)
        const uint32_t c0 = s.t.child0[base + node];
        const float parent = (float)vis;
        const bool parent_loss = ev.tag == TZ_EVAL_LOSS;
        float best_score = 0.0f;
        int best_i = -1;
        if constexpr (RULE == TZ_SELECT_PUCT) {
            // select_with_puct, policy.rs:78-95
            const float er = tz_logf(((1.0f + parent) + 500.0f) / 500.0f) + 4.0f;  // policy.rs:143-145
            const float sq = sqrtf(parent);
            for (int i = l; i < nc; i += 64) {
                const size_t ci = base + c0 + i;
                const Ev ce{s.t.eval_tag[ci], s.t.eval_bits[ci]};
                if (!(parent_loss || ce.tag != TZ_EVAL_WIN)) continue;
                const float q = ev_to_notnan(ev_negate(ce));
                const float puct = ((er * s.t.prob[ci]) * sq) / (1.0f + (float)s.t.visits[ci]);
                const float score = (q + puct) + s.t.std_dev[ci] * beta;
                if (best_i < 0 || !(score < best_score)) {
                    best_score = score;
                    best_i = i;
                }
            }
        } else if constexpr (RULE == TZ_SELECT_UCT) {
            // select_with_uct, policy.rs:104-117.  A node with children has vis >= 2, so ln > 0 and an unvisited child scores
            // ln(N) / 0 = +inf: those are taken from the last index to the first.
            const float lnp = tz_logf(parent);
            bool nan = false;
            for (int i = l; i < nc; i += 64) {
                const size_t ci = base + c0 + i;
                const Ev ce{s.t.eval_tag[ci], s.t.eval_bits[ci]};
                if (!(parent_loss || ce.tag != TZ_EVAL_WIN)) continue;
                const float q = ev_to_notnan(ev_negate(ce));
                const float uct = 1.0f * sqrtf(lnp / (float)s.t.visits[ci]);  // policy.rs:158-164
                const float score = (q + uct) + s.t.std_dev[ci] * beta;
                nan = nan || !(score == score);
                if (best_i < 0 || !(score < best_score)) {
                    best_score = score;
                    best_i = i;
                }
            }
            if (__any(nan)) {  // NotNan::new panics, policy.rs:113
                if (l == 0) atomicMax(s.error_flag, 8);
                return 2;
            }
        } else {
            // select_with_improved_policy, policy.rs:57-69; beta is not read
            // The row holds a default max_actions, so this is a pure guard: a node with more children was expanded under a larger
            // max_actions than the row allows.  Flag 3 is the one gen_moves raises for a position with more legal moves than
            // max_actions, and the host words it that way.
            if (nc > SelectRow<N, RULE>::LEN) {
                if (l == 0) atomicMax(s.error_flag, 3);
                return 2;
            }
            uint32_t vm = 0;  // most_visited_count, policy.rs:23-29
            for (int i = l; i < nc; i += 64) {
                const uint32_t v = s.t.visits[base + c0 + i];
                vm = v > vm ? v : vm;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)vm, d);
                vm = o > vm ? o : vm;
            }
            const float sqv = sqrtf((float)vm);
            // improved_policy, policy.rs:36-48: p = sigma_improve(completed, std_dev, 0.0, vmax) + logit over every child
            bool nan = false;
            float mx = -3.4028235e38f;
            for (int i = l; i < nc; i += 64) {
                const size_t ci = base + c0 + i;
                const Ev ce{s.t.eval_tag[ci], s.t.eval_bits[ci]};
                const bool needs_init = s.t.nchild[ci] == 0 && !ev_known(ce);
                // The reference's `.into()` here is From<Eval> for NotNan<f32> (ev_to_notnan); ev_to_f32 gives the same bits:
                // the two differ only for a Value, which ev_to_f32 multiplies by powif(d, 0) == 1.0f, and 1.0f * x == x.
                const float completed = ev_to_f32(needs_init ? ev : ev_negate(ce));
                const float p = ((completed + s.t.std_dev[ci] * 0.0f) * sqv) + s.t.logit[ci];  // policy.rs:131-138
                nan = nan || !(p == p);
                prow[i] = p;
                mx = p > mx ? p : mx;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float o = __shfl_xor(mx, d);
                mx = o > mx ? o : mx;
            }
            if (__any(nan)) {  // NotNan, policy.rs:37
                if (l == 0) atomicMax(s.error_flag, 8);
                return 2;
            }
            // softmax, policy.rs:10-19: each lane rewrites the slots it wrote; the sum is the sequential f32 sum in child order,
            // read from LDS by every lane (same address: a broadcast), as in expand_kernel
            for (int i = l; i < nc; i += 64) prow[i] = tz_expf(prow[i] - mx);
            __syncthreads();
            float sum = 0.0f;
            for (int i = 0; i < nc; i++) sum = sum + prow[i];
            const float denom = (float)(vis + 1u);  // (self.visit_count + 1) as f32, policy.rs:65
            for (int i = l; i < nc; i += 64) {
                const size_t ci = base + c0 + i;
                if (!(parent_loss || s.t.eval_tag[ci] != TZ_EVAL_WIN)) continue;
                const float score = prow[i] / sum - (float)s.t.visits[ci] / denom;
                nan = nan || !(score == score);
                if (best_i < 0 || !(score < best_score)) {
                    best_score = score;
                    best_i = i;
                }
            }
            if (__any(nan)) {
                if (l == 0) atomicMax(s.error_flag, 8);
                return 2;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float os = __shfl_xor(best_score, d);
            const int oi = __shfl_xor(best_i, d);
            if (oi >= 0 && (best_i < 0 || os > best_score || (os == best_score && oi > best_i))) {
                best_score = os;
                best_i = oi;
            }
        }
        if (best_i < 0) {  // reference: expect("there should always be a child to simulate")
            if (l == 0) atomicMax(s.error_flag, 4);
            return 2;
        }
        node = c0 + (uint32_t)best_i;
        apply_move<N>(&env, s.t.action[base + node]);
        __syncthreads();
    }
}

template <int N, int RULE>
__global__ __launch_bounds__(64) void descend_kernel(SearchDev s, int from_start) {
    constexpr int NN = N * N;
    const int g = blockIdx.x, l = lane_id();
    __shared__ tz_state env;
    __shared__ uint32_t tnode[TZ_MAX_DEPTH];
    __shared__ uint32_t tvis[TZ_MAX_DEPTH];
    __shared__ uint8_t reach[NN * 4];
    float* prow = nullptr;
    if constexpr (RULE == TZ_SELECT_IMPROVED) {
        __shared__ float row[SelectRow<N, RULE>::LEN];
        prow = row;
    }
    load_state(&env, &s.env[g]);
    const size_t base = slab_base(s, s.bank[g], g);
    uint32_t node = 0;
    float beta = s.betas[g];
    if (from_start) {
        node = (uint32_t)s.start_node[g];
        beta = 0.0f;  // batched.rs:279
    }
    __syncthreads();
    if (from_start && node != 0) {
        apply_move<N>(&env, s.t.action[base + node]);
        __syncthreads();
    }
    int depth = 0;
    Ev known{0, 0};
    const int kind = forward_walk<N, RULE>(s, base, env, tnode, tvis, node, beta, depth, known, prow);  // 0 known, 1 needs network, 2 error
    __syncthreads();
    if (kind == 0) {
        // backward_known_eval, mcts.rs:141-163: the leaf itself is not updated
        backup(s, base, tnode, tvis, depth - 1, known, 0.0f, known);
        if (l == 0) {
            s.leaf_kind[g] = 0;
            s.traj_len[g] = 0;
        }
        return;
    }
    if (kind == 2) {
        if (l == 0) {
            s.leaf_kind[g] = 0;
            s.traj_len[g] = 0;
        }
        return;
    }
    // NeedsNetwork: env.populate_actions (batched.rs:84) + hand the leaf position to the net
    uint16_t* acts = s.leaf_act + (size_t)g * s.max_actions;
    const int nact = gen_moves<N>(&env, reach, acts, s.max_actions);
    if (nact > s.max_actions) {
        // gen_moves wrote the moves that fit and left the rest of the row as it was: such a leaf is not expanded (its game stands
        // still until set_positions replaces it), the other games go on
        if (l == 0) {
            atomicMax(s.error_flag, 3);
            s.leaf_kind[g] = 0;
            s.traj_len[g] = 0;
        }
        return;
    }
    {
        const uint32_t* a = reinterpret_cast<const uint32_t*>(&env);
        uint32_t* b = reinterpret_cast<uint32_t*>(&s.leaf_env[g]);
        for (int i = l; i < (int)(sizeof(tz_state) / 4); i += 64) b[i] = a[i];
    }
    for (int i = l; i < depth; i += 64) s.traj[(size_t)g * TZ_MAX_DEPTH + i] = tnode[i];
    if (l == 0) {
        s.leaf_kind[g] = 1;
        s.leaf_nact[g] = (uint16_t)nact;
        s.traj_len[g] = (uint32_t)depth;
    }
}

// games whose leaf needs the network, in ascending game order (batched.rs:66-90 filter_map order)
__global__ __launch_bounds__(1024) void compact_kernel(SearchDev s) {
    __shared__ int wsum[16];
    __shared__ int carry;
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int chunk = 0; chunk < s.batch; chunk += 1024) {
        const int g = chunk + tid;
        const int f = (g < s.batch && s.leaf_kind[g] == 1) ? 1 : 0;
        const int incl = wave_incl_scan(f);
        if (l == 63) wsum[w] = incl;
        __syncthreads();
        int off = carry;
        for (int i = 0; i < w; i++) off += wsum[i];
        if (f) s.nn_game[off + incl - 1] = g;
        __syncthreads();
        if (tid == 1023) carry = off + incl;
        __syncthreads();
    }
    if (tid == 0) {
        *s.nn_count = carry;
        s.counters[0] += (unsigned long long)s.batch;
        s.counters[1] += (unsigned long long)carry;
    }
}

// ---------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(64) void expand_kernel(SearchDev s, NetOut out) {
    constexpr int NN = N * N;
    const int slot = blockIdx.x, l = lane_id();
    if (slot >= *s.nn_count) return;
    const int g = s.nn_game[slot];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* tnode = reinterpret_cast<uint32_t*>(smem);
    uint32_t* tvis = tnode + TZ_MAX_DEPTH;
    float* lg = reinterpret_cast<float*>(tvis + TZ_MAX_DEPTH);
    float* ex = lg + s.max_actions;
    const size_t base = slab_base(s, s.bank[g], g);
    const int len = (int)s.traj_len[g];
    for (int i = l; i < len; i += 64) {
        const uint32_t nd = s.traj[(size_t)g * TZ_MAX_DEPTH + i];
        tnode[i] = nd;
        tvis[i] = s.t.visits[base + nd];
    }
    const int nact = s.leaf_nact[g];
    const uint16_t* acts = s.leaf_act + (size_t)g * s.max_actions;
    // Agent::policy_value_uncertainty outputs for this leaf
    float value = 0.0f, variance = 0.0f;
    if (s.agent_kind == TZ_AGENT_NET) {
        value = out.value[slot];
        variance = out.variance[slot];
    } else if (s.agent_kind == TZ_AGENT_SIMPLE) {  // agent.rs:66-70
        __shared__ tz_state le;
        load_state(&le, &s.leaf_env[g]);
        __syncthreads();
        const int fd = flat_diff<N>(&le) - s.half_komi / 2;
        value = (float)fd / (float)NN;
        if (le.to_move == 1) value = -value;
    }
    bool nan = false;
    float mx = -3.4028235e38f;
    for (int i = l; i < nact; i += 64) {
        const int a = acts[i];
        float x;
        if (s.agent_kind == TZ_AGENT_NET) {
            x = out.policy[((size_t)slot * NN + (a % NN)) * out.policy_stride + a / NN];
        } else if (s.agent_kind == TZ_AGENT_DUMMY) {
            x = 1.0f;
        } else {
            const int ch = a / NN;
            x = ch == 0 ? 4.0f : ch == 1 ? 2.0f : ch == 2 ? 3.0f : 1.0f;  // agent.rs:73-80
        }
        nan = nan || !(x == x);
        lg[i] = x;
        mx = x > mx ? x : mx;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(mx, d);
        mx = o > mx ? o : mx;
    }
    if (__any(nan) || !(value == value) || !(variance == variance)) {
        if (l == 0) atomicMax(s.error_flag, 7);
        return;
    }
    // softmax over the legal moves only, policy.rs:10-19 (sequential f32 sum)
    for (int i = l; i < nact; i += 64) ex[i] = tz_expf(lg[i] - mx);
    __syncthreads();
    float sum = 0.0f;
    for (int i = 0; i < nact; i++) sum = sum + ex[i];
    // leaf update, mcts.rs:190-196
    const uint32_t leaf = tnode[len - 1];
    const float n = (float)tvis[len - 1];
    float mean = tz_bits_to_float(s.t.eval_bits[base + leaf]);
    mean = mean + (-mean + value) / n;
    float sd = s.t.std_dev[base + leaf];
    sd = sd + (-sd + sqrtf(variance)) / n;
    const uint32_t c0 = s.alloc[g];
    // The reference's trees live on the heap and are unbounded; a game's pool here is not.  A full pool is either an
    // error (strict) or the leaf is evaluated and backed up without getting children: it stays a leaf, is simply
    // evaluated again when it is reached again, and the next `step` compacts the kept subtree and frees the rest.
    const bool full = c0 + (uint32_t)nact > (uint32_t)s.cap;
    if (full && s.strict_capacity) {
        if (l == 0) atomicMax(s.error_flag, 1);
        return;
    }
    // children, node/mod.rs:66-79
    const uint32_t child_bits = tz_float_to_bits(-mean);
    for (int i = l; i < (full ? 0 : nact); i += 64) {
        const size_t ci = base + c0 + i;
        s.t.eval_tag[ci] = TZ_EVAL_VALUE;
        s.t.eval_bits[ci] = child_bits;
        s.t.visits[ci] = 0;
        s.t.prob[ci] = ex[i] / sum;
        s.t.logit[ci] = lg[i];
        s.t.std_dev[ci] = sd;
        s.t.child0[ci] = 0;
        s.t.nchild[ci] = 0;
        s.t.action[ci] = acts[i];
    }
    if (l == 0) {
        s.t.eval_bits[base + leaf] = tz_float_to_bits(mean);
        s.t.std_dev[base + leaf] = sd;
        if (full) {
            atomicAdd(&s.counters[2], 1ull);
        } else {
            s.alloc[g] = c0 + (uint32_t)nact;
            s.t.child0[base + leaf] = c0;
            s.t.nchild[base + leaf] = (uint16_t)nact;
        }
    }
    __syncthreads();
    backup(s, base, tnode, tvis, len - 1, ev_value(value * TZ_DISCOUNT), variance * TZ_DISCOUNT * TZ_DISCOUNT, ev_value(mean));
}

// ---------------------------------------------------------------------------------------------
// Node::simulate_batch, mcts.rs:268-328, on every root of the handle: descend_batch_kernel (the forward loop of a round),
// compact_batch_kernel, the network, leaf_policy_kernel (softmax per collected leaf), expand_batch_kernel (backward_network_eval per
// tree in collection order).  Leaf slot (g, j) of LeafBatchDev is g * leaves + j.
//
// One wave per tree runs the forward loop of mcts.rs:281-300: up to 4 * leaves forwards, a Known result backed up at once (:284),
// a leaf that needs the network written to the tree's next slot, until `leaves` are collected (:297).  A forward reads the visit
// counts and solver results lane 0 stored in the forwards before it, hence the fence and barrier between trajectories.
template <int N, int RULE>
__global__ __launch_bounds__(64) void descend_batch_kernel(SearchDev s, LeafBatchDev b) {
    constexpr int NN = N * N;
    const int g = blockIdx.x, l = lane_id();
    __shared__ tz_state root_env;
    __shared__ tz_state env;
    __shared__ uint32_t tnode[TZ_MAX_DEPTH];
    __shared__ uint32_t tvis[TZ_MAX_DEPTH];
    __shared__ uint8_t reach[NN * 4];
    float* prow = nullptr;
    if constexpr (RULE == TZ_SELECT_IMPROVED) {
        __shared__ float row[SelectRow<N, RULE>::LEN];
        prow = row;
    }
    load_state(&root_env, &s.env[g]);
    const size_t base = slab_base(s, s.bank[g], g);
    const float beta = s.betas[g];
    int collected = 0, forwards = 0;
    __syncthreads();
    for (int f = 0; f < 4 * b.leaves && collected < b.leaves; f++) {
        load_state(&env, &root_env);  // env.clone(), mcts.rs:283
        __syncthreads();
        int depth = 0;
        Ev known{0, 0};
        const int kind = forward_walk<N, RULE>(s, base, env, tnode, tvis, 0, beta, depth, known, prow);
        __syncthreads();
        forwards++;
        if (kind == 2) break;
        if (kind == 0) {
            backup(s, base, tnode, tvis, depth - 1, known, 0.0f, known);  // backward_known_eval, mcts.rs:141-163
        } else {
            const size_t slot = (size_t)g * b.leaves + collected;
            uint16_t* acts = b.act + slot * s.max_actions;
            const int nact = gen_moves<N>(&env, reach, acts, s.max_actions);  // env.populate_actions, mcts.rs:289
            if (nact > s.max_actions) {  // not collected: the row holds only the moves that fit (see descend_kernel)
                if (l == 0) atomicMax(s.error_flag, 3);
                break;
            }
            {
                const uint32_t* a = reinterpret_cast<const uint32_t*>(&env);
                uint32_t* d = reinterpret_cast<uint32_t*>(&b.env[slot]);
                for (int i = l; i < (int)(sizeof(tz_state) / 4); i += 64) d[i] = a[i];
            }
            for (int i = l; i < depth; i += 64) b.traj[slot * TZ_MAX_DEPTH + i] = tnode[i];
            if (l == 0) {
                b.nact[slot] = (uint16_t)nact;
                b.traj_len[slot] = (uint32_t)depth;
            }
            collected++;
        }
        __threadfence_block();
        __syncthreads();
    }
    if (l == 0) {
        b.count[g] = collected;
        b.forwards[g] = forwards;
    }
}

// The net's index list: tree g's leaves take the net slots [offset[g], offset[g] + count[g]) in collection order, trees in
// ascending order.  Also the counters: simulations grow by the forwards made, nn leaf evals by the leaves collected.
__global__ __launch_bounds__(1024) void compact_batch_kernel(SearchDev s, LeafBatchDev b) {
    __shared__ int wsum[16];
    __shared__ int carry;
    __shared__ unsigned long long fsum;
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    if (tid == 0) {
        carry = 0;
        fsum = 0;
    }
    __syncthreads();
    for (int chunk = 0; chunk < s.batch; chunk += 1024) {
        const int g = chunk + tid;
        const int c = g < s.batch ? b.count[g] : 0;
        if (g < s.batch) atomicAdd(&fsum, (unsigned long long)b.forwards[g]);
        const int incl = wave_incl_scan(c);
        if (l == 63) wsum[w] = incl;
        __syncthreads();
        int off = carry;
        for (int i = 0; i < w; i++) off += wsum[i];
        if (g < s.batch) b.offset[g] = off + incl - c;
        __syncthreads();
        if (tid == 1023) carry = off + incl;
        __threadfence_block();
        __syncthreads();
    }
    const int slots = s.batch * b.leaves;
    for (int i = tid; i < slots; i += 1024) {
        const int g = i / b.leaves, j = i - g * b.leaves;
        if (j < b.count[g]) b.index[b.offset[g] + j] = i;
    }
    if (tid == 0) {
        *s.nn_count = carry;
        s.counters[0] += fsum;
        s.counters[1] += (unsigned long long)carry;
    }
}

// Agent::policy_value_uncertainty outputs and softmax (policy.rs:10-19) of every collected leaf, one wave per slot: a leaf's
// probabilities do not depend on the other leaves.  The arithmetic is expand_kernel's: the sum is the sequential f32 sum.
template <int N>
__global__ __launch_bounds__(64) void leaf_policy_kernel(SearchDev s, LeafBatchDev b, NetOut out) {
    constexpr int NN = N * N;
    const int slot = blockIdx.x, l = lane_id();
    const int g = slot / b.leaves, j = slot - g * b.leaves;
    if (j >= b.count[g]) return;
    const int k = b.offset[g] + j;  // the leaf's slot in the net's outputs
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* lg = reinterpret_cast<float*>(smem);
    float* ex = lg + s.max_actions;
    const int nact = b.nact[slot];
    const uint16_t* acts = b.act + (size_t)slot * s.max_actions;
    float value = 0.0f, variance = 0.0f;
    if (s.agent_kind == TZ_AGENT_NET) {
        value = out.value[k];
        variance = out.variance[k];
    } else if (s.agent_kind == TZ_AGENT_SIMPLE) {  // agent.rs:66-70
        __shared__ tz_state le;
        load_state(&le, &b.env[slot]);
        __syncthreads();
        const int fd = flat_diff<N>(&le) - s.half_komi / 2;
        value = (float)fd / (float)NN;
        if (le.to_move == 1) value = -value;
    }
    bool nan = false;
    float mx = -3.4028235e38f;
    for (int i = l; i < nact; i += 64) {
        const int a = acts[i];
        float x;
        if (s.agent_kind == TZ_AGENT_NET) {
            x = out.policy[((size_t)k * NN + (a % NN)) * out.policy_stride + a / NN];
        } else if (s.agent_kind == TZ_AGENT_DUMMY) {
            x = 1.0f;
        } else {
            const int ch = a / NN;
            x = ch == 0 ? 4.0f : ch == 1 ? 2.0f : ch == 2 ? 3.0f : 1.0f;  // agent.rs:73-80
        }
        nan = nan || !(x == x);
        lg[i] = x;
        mx = x > mx ? x : mx;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_xor(mx, d);
        mx = o > mx ? o : mx;
    }
    const bool bad = __any(nan) || !(value == value) || !(variance == variance);
    if (bad) {
        if (l == 0) {
            atomicMax(s.error_flag, 7);
            b.bad[slot] = 1;
        }
        return;
    }
    for (int i = l; i < nact; i += 64) ex[i] = tz_expf(lg[i] - mx);
    __syncthreads();
    float sum = 0.0f;
    for (int i = 0; i < nact; i++) sum = sum + ex[i];
    float* lo = b.logit + (size_t)slot * s.max_actions;
    float* po = b.prob + (size_t)slot * s.max_actions;
    for (int i = l; i < nact; i += 64) {
        lo[i] = lg[i];
        po[i] = ex[i] / sum;
    }
    if (l == 0) {
        b.value[slot] = value;
        b.variance[slot] = variance;
        b.bad[slot] = 0;
    }
}

// backward_network_eval (mcts.rs:171-225) for a tree's leaves strictly in collection order (mcts.rs:307-327): each backup changes
// what the next one reads.  n of update_mean_value / update_standard_deviation is the node's visit_count now, which already holds
// every forward of the round.  A leaf collected more than once in a round (always on a fresh root) has children from its first
// expansion; the reference replaces `children` each time (mcts.rs:199-217), and since no forward of the round went below the leaf
// the new children differ from the old only in the fields rewritten here, in the same slots.
__global__ __launch_bounds__(64) void expand_batch_kernel(SearchDev s, LeafBatchDev b) {
    const int g = blockIdx.x, l = lane_id();
    __shared__ uint32_t tnode[TZ_MAX_DEPTH];
    __shared__ uint32_t tvis[TZ_MAX_DEPTH];
    const size_t base = slab_base(s, s.bank[g], g);
    const int count = b.count[g];
    for (int j = 0; j < count; j++) {
        const size_t slot = (size_t)g * b.leaves + j;
        if (b.bad[slot]) return;  // NaN from the agent: error 7 is set, the reference panics (mcts.rs:194)
        const int len = (int)b.traj_len[slot];
        for (int i = l; i < len; i += 64) {
            const uint32_t nd = b.traj[slot * TZ_MAX_DEPTH + i];
            tnode[i] = nd;
            tvis[i] = s.t.visits[base + nd];
        }
        __syncthreads();
        const int nact = b.nact[slot];
        const uint16_t* acts = b.act + slot * s.max_actions;
        const float* lg = b.logit + slot * s.max_actions;
        const float* pr = b.prob + slot * s.max_actions;
        const float value = b.value[slot], variance = b.variance[slot];
        // leaf update, mcts.rs:190-196
        const uint32_t leaf = tnode[len - 1];
        const float n = (float)tvis[len - 1];
        float mean = tz_bits_to_float(s.t.eval_bits[base + leaf]);
        mean = mean + (-mean + value) / n;
        float sd = s.t.std_dev[base + leaf];
        sd = sd + (-sd + sqrtf(variance)) / n;
        const bool again = s.t.nchild[base + leaf] != 0;  // expanded by an earlier leaf of this round
        const uint32_t c0 = again ? s.t.child0[base + leaf] : s.alloc[g];
        const bool full = !again && c0 + (uint32_t)nact > (uint32_t)s.cap;  // as expand_kernel
        if (full && s.strict_capacity) {
            if (l == 0) atomicMax(s.error_flag, 1);
            return;
        }
        // children, node/mod.rs:66-79
        const uint32_t child_bits = tz_float_to_bits(-mean);
        for (int i = l; i < (full ? 0 : nact); i += 64) {
            const size_t ci = base + c0 + i;
            s.t.eval_tag[ci] = TZ_EVAL_VALUE;
            s.t.eval_bits[ci] = child_bits;
            s.t.visits[ci] = 0;
            s.t.prob[ci] = pr[i];
            s.t.logit[ci] = lg[i];
            s.t.std_dev[ci] = sd;
            if (!again) {
                s.t.child0[ci] = 0;
                s.t.nchild[ci] = 0;
                s.t.action[ci] = acts[i];
            }
        }
        if (l == 0) {
            s.t.eval_bits[base + leaf] = tz_float_to_bits(mean);
            s.t.std_dev[base + leaf] = sd;
            if (full) {
                atomicAdd(&s.counters[2], 1ull);
            } else if (!again) {
                s.alloc[g] = c0 + (uint32_t)nact;
                s.t.child0[base + leaf] = c0;
                s.t.nchild[base + leaf] = (uint16_t)nact;
            }
        }
        __syncthreads();
        backup(s, base, tnode, tvis, len - 1, ev_value(value * TZ_DISCOUNT), variance * TZ_DISCOUNT * TZ_DISCOUNT, ev_value(mean));
        __threadfence_block();
        __syncthreads();
    }
}

// noise.rs:10-26 with the sample supplied by the caller
__global__ __launch_bounds__(64) void noise_kernel(SearchDev s, const float* noise, int amax, float ratio) {
    const int g = blockIdx.x, l = lane_id();
    const size_t base = slab_base(s, s.bank[g], g);
    const int nc = s.t.nchild[base];
    const bool known = s.t.eval_tag[base] != TZ_EVAL_VALUE;
    if (nc == 0 && !known) {
        if (l == 0) atomicMax(s.error_flag, 6);
        return;
    }
    const uint32_t c0 = s.t.child0[base];
    const float keep = 1.0f - ratio;
    for (int i = l; i < nc && i < amax; i += 64) {
        const size_t ci = base + c0 + i;
        const float p = s.t.prob[ci] * keep + noise[(size_t)g * amax + i] * ratio;
        s.t.prob[ci] = p;
        s.t.logit[ci] = tz_logf(p);
    }
}

template <int N>
__global__ __launch_bounds__(64) void root_info_kernel(SearchDev s, tz_root_info* out) {
    const int g = blockIdx.x, l = lane_id();
    __shared__ tz_state env;
    load_state(&env, &s.env[g]);
    __syncthreads();
    const int t = terminal<N>(&env);
    if (l != 0) return;
    const size_t base = slab_base(s, s.bank[g], g);
    tz_root_info r;
    r.visit_count = s.t.visits[base];
    r.n_children = s.t.nchild[base];
    r.eval_tag = s.t.eval_tag[base];
    r.is_terminal_env = t != TZ_TERMINAL_NONE;
    r.ply = env.ply;
    r.eval.ply = s.t.eval_bits[base];
    r.std_dev = s.t.std_dev[base];
    r.logit = s.t.logit[base];
    r.probability = s.t.prob[base];
    out[g] = r;
}

__global__ __launch_bounds__(64) void root_children_kernel(SearchDev s, int amax, uint16_t* move_idx, uint32_t* visits,
                                                           uint8_t* eval_tag, uint32_t* eval_bits, float* logit,
                                                           float* prob, float* std_dev) {
    const int g = blockIdx.x, l = lane_id();
    const size_t base = slab_base(s, s.bank[g], g);
    const int nc = s.t.nchild[base];
    const uint32_t c0 = s.t.child0[base];
    for (int i = l; i < amax; i += 64) {
        const size_t o = (size_t)g * amax + i;
        const bool in = i < nc;
        const size_t ci = base + c0 + i;
        if (move_idx) move_idx[o] = in ? s.t.action[ci] : 0;
        if (visits) visits[o] = in ? s.t.visits[ci] : 0;
        if (eval_tag) eval_tag[o] = in ? s.t.eval_tag[ci] : 0;
        if (eval_bits) eval_bits[o] = in ? s.t.eval_bits[ci] : 0;
        if (logit) logit[o] = in ? s.t.logit[ci] : 0.0f;
        if (prob) prob[o] = in ? s.t.prob[ci] : 0.0f;
        if (std_dev) std_dev[o] = in ? s.t.std_dev[ci] : 0.0f;
    }
}

// A node below the root (Node.children is a public field of the reference, node/mod.rs:14-23, read by puzzle / visualize_search):
// one wave walks `path` (move indices) from game g's root; status = -1 found, else the depth at which the path left the tree.
// out_words: [0] visits [1] nchild [2] tag [3] bits [4] std_dev [5] logit [6] prob; children rows as root_children_kernel.
__global__ __launch_bounds__(64) void node_kernel(SearchDev s, int g, const uint16_t* path, int len, uint32_t* out_words, int* status,
                                                  int amax, uint16_t* move_idx, uint32_t* visits, uint8_t* eval_tag, uint32_t* eval_bits,
                                                  float* logit, float* prob, float* std_dev) {
    const int l = lane_id();
    const size_t base = slab_base(s, s.bank[g], g);
    size_t node = base;
    for (int d = 0; d < len; d++) {
        const int nc = s.t.nchild[node];
        const uint32_t c0 = s.t.child0[node];
        int found = -1;
        for (int i0 = 0; i0 < nc && found < 0; i0 += 64) {
            const int i = i0 + l;
            const bool hit = i < nc && s.t.action[base + c0 + i] == path[d];
            const unsigned long long m = __ballot(hit);
            if (m) found = i0 + __ffsll((long long)m) - 1;
        }
        if (found < 0) {
            if (l == 0) *status = d;
            return;
        }
        node = base + c0 + found;
    }
    const int nc = s.t.nchild[node];
    const uint32_t c0 = s.t.child0[node];
    if (l == 0) {
        *status = -1;
        out_words[0] = s.t.visits[node];
        out_words[1] = (uint32_t)nc;
        out_words[2] = s.t.eval_tag[node];
        out_words[3] = s.t.eval_bits[node];
        out_words[4] = __float_as_uint(s.t.std_dev[node]);
        out_words[5] = __float_as_uint(s.t.logit[node]);
        out_words[6] = __float_as_uint(s.t.prob[node]);
    }
    for (int i = l; i < amax; i += 64) {
        const bool in = i < nc;
        const size_t ci = base + c0 + i;
        move_idx[i] = in ? s.t.action[ci] : 0;
        visits[i] = in ? s.t.visits[ci] : 0;
        eval_tag[i] = in ? s.t.eval_tag[ci] : 0;
        eval_bits[i] = in ? s.t.eval_bits[ci] : 0;
        logit[i] = in ? s.t.logit[ci] : 0.0f;
        prob[i] = in ? s.t.prob[ci] : 0.0f;
        std_dev[i] = in ? s.t.std_dev[ci] : 0.0f;
    }
}

// Node::select_best_action, node/mod.rs:132-161, of the node at slab index `node` (base + index) with children [c0, c0 + nc), nc > 0:
// the position of the chosen child among them (uniform over the wave)
__device__ __forceinline__ int select_best_child(const SearchDev& s, size_t base, size_t node, uint32_t c0, int nc) {
    const int l = lane_id();
    int pick;
    if (s.t.eval_tag[node] != TZ_EVAL_VALUE) {  // solved: first minimum child evaluation
        Ev best{0, 0};
        int best_i = 0x7fffffff;
        // Selects, not a branch around `best = e`: with more than 64 children the branch form was compiled (hipcc of ROCm 7.2, gfx950, -O3)
        // into a loop whose later iterations replaced best.bits alone and kept the tag and the index of the lane's first child, so
        // a solved node whose best child lay beyond its first 64 answered with another move (tests/test_gpu_action_capacity.py).
        for (int i = l; i < nc; i += 64) {
            const Ev e{s.t.eval_tag[base + c0 + i], s.t.eval_bits[base + c0 + i]};
            const bool take = best_i == 0x7fffffff || ev_cmp(e, best) < 0;
            best.tag = take ? e.tag : best.tag;
            best.bits = take ? e.bits : best.bits;
            best_i = take ? i : best_i;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const Ev o{(uint32_t)__shfl_xor((int)best.tag, d), (uint32_t)__shfl_xor((int)best.bits, d)};
            const int oi = __shfl_xor(best_i, d);
            if (oi != 0x7fffffff) {
                const int c = best_i == 0x7fffffff ? -1 : ev_cmp(o, best);
                if (c < 0 || (c == 0 && oi < best_i)) {
                    best = o;
                    best_i = oi;
                }
            }
        }
        pick = best_i;
    } else {  // most visited (last max); all zero -> highest prior (last max)
        uint32_t bv = 0;
        int bvi = -1;
        float bp = 0.0f;
        int bpi = -1;
        for (int i = l; i < nc; i += 64) {
            const uint32_t v = s.t.visits[base + c0 + i];
            const float p = s.t.prob[base + c0 + i];
            if (bvi < 0 || v >= bv) {
                bv = v;
                bvi = i;
            }
            if (bpi < 0 || !(p < bp)) {
                bp = p;
                bpi = i;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t ov = (uint32_t)__shfl_xor((int)bv, d);
            const int ovi = __shfl_xor(bvi, d);
            if (ovi >= 0 && (bvi < 0 || ov > bv || (ov == bv && ovi > bvi))) {
                bv = ov;
                bvi = ovi;
            }
            const float op = __shfl_xor(bp, d);
            const int opi = __shfl_xor(bpi, d);
            if (opi >= 0 && (bpi < 0 || op > bp || (op == bp && opi > bpi))) {
                bp = op;
                bpi = opi;
            }
        }
        pick = bv == 0 ? bpi : bvi;
    }
    return pick;
}

__global__ __launch_bounds__(64) void select_best_kernel(SearchDev s, uint16_t* out) {
    const int g = blockIdx.x, l = lane_id();
    const size_t base = slab_base(s, s.bank[g], g);
    const int nc = s.t.nchild[base];
    const uint32_t c0 = s.t.child0[base];
    if (nc == 0) {
        if (l == 0) out[g] = 0xFFFF;
        return;
    }
    const int pick = select_best_child(s, base, base, c0, nc);
    if (l == 0) out[g] = s.t.action[base + c0 + pick];
}

// Node::principal_variation, node/mod.rs:40-62, 87-90: one wave follows select_best_action from game g's root until a node
// needs initialisation or is terminal.  moves[cap] receives the first cap moves, *len the whole length.
__global__ __launch_bounds__(64) void principal_variation_kernel(SearchDev s, int g, uint16_t* moves, int cap, int* len) {
    const int l = lane_id();
    const size_t base = slab_base(s, s.bank[g], g);
    size_t node = base;
    int d = 0;
    for (; d < TZ_MAX_DEPTH; d++) {
        const int nc = s.t.nchild[node];
        const bool known = s.t.eval_tag[node] != TZ_EVAL_VALUE;
        if ((nc == 0 && !known) || (known && s.t.eval_bits[node] == 0)) break;
        if (nc == 0) break;  // a solved node whose children the tree does not hold: the reference would panic (mod.rs:139)
        const uint32_t c0 = s.t.child0[node];
        const int pick = select_best_child(s, base, node, c0, nc);
        node = base + c0 + pick;
        if (l == 0 && d < cap) moves[d] = s.t.action[node];
    }
    if (l == 0) *len = d;
}

__device__ __forceinline__ void copy_node(const SearchDev& s, size_t dst, size_t src) {
    s.t.eval_tag[dst] = s.t.eval_tag[src];
    s.t.eval_bits[dst] = s.t.eval_bits[src];
    s.t.visits[dst] = s.t.visits[src];
    s.t.prob[dst] = s.t.prob[src];
    s.t.logit[dst] = s.t.logit[src];
    s.t.std_dev[dst] = s.t.std_dev[src];
    s.t.nchild[dst] = s.t.nchild[src];
    s.t.action[dst] = s.t.action[src];
    s.t.child0[dst] = 0;
}

// BatchedMCTS::step, batched.rs:131-144: descend (subtree reuse) + env.step, skipped for terminal
// roots.  The kept subtree is copied breadth-first into the game's other bank.
template <int N>
__global__ __launch_bounds__(64) void step_kernel(SearchDev s, const uint16_t* actions) {
    const int g = blockIdx.x, l = lane_id();
    __shared__ tz_state env;
    const int sbank = s.bank[g], dbank = 1 - sbank;
    const size_t sb = slab_base(s, sbank, g), db = slab_base(s, dbank, g);
    if (s.t.eval_tag[sb] != TZ_EVAL_VALUE && s.t.eval_bits[sb] == 0) return;  // root.is_terminal()
    const int action = actions[g];
    const int nc = s.t.nchild[sb];
    const uint32_t c0 = s.t.child0[sb];
    int found = -1;
    for (int i = l; i < nc; i += 64)
        if (s.t.action[sb + c0 + i] == action) found = i;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(found, d);
        found = o > found ? o : found;
    }
    uint32_t* bsrc = s.bfs_src + (size_t)g * s.cap;
    uint32_t count = 1;
    if (found < 0) {
        if (l == 0) write_default_node(s, db);
    } else {
        if (l == 0) {
            copy_node(s, db, sb + c0 + found);
            bsrc[0] = c0 + (uint32_t)found;
        }
        __threadfence_block();
        __syncthreads();
        uint32_t head = 0;
        bool overflow = false;
        while (head < count && !overflow) {
            const uint32_t i = head + l;
            const bool have = i < count;
            const uint32_t src = have ? bsrc[i] : 0;
            const int cn = have ? (int)s.t.nchild[sb + src] : 0;
            const uint32_t cc0 = have ? s.t.child0[sb + src] : 0;
            const int incl = wave_incl_scan(cn);
            const uint32_t off = count + (uint32_t)(incl - cn);
            const uint32_t total = (uint32_t)__shfl(incl, 63);
            if (count + total > (uint32_t)s.cap) {
                overflow = true;
                break;
            }
            if (have && cn) s.t.child0[db + i] = off;
            unsigned long long m = __ballot(cn > 0);
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const uint32_t jc0 = (uint32_t)__shfl((int)cc0, j);
                const int jn = __shfl(cn, j);
                const uint32_t joff = (uint32_t)__shfl((int)off, j);
                for (int k = l; k < jn; k += 64) {
                    copy_node(s, db + joff + k, sb + jc0 + k);
                    bsrc[joff + k] = jc0 + k;
                }
            }
            __threadfence_block();
            __syncthreads();
            const uint32_t processed = count - head < 64 ? count - head : 64;
            head += processed;
            count += total;
        }
        if (overflow && l == 0) atomicMax(s.error_flag, 1);
    }
    load_state(&env, &s.env[g]);
    __syncthreads();
    apply_move<N>(&env, action);
    __syncthreads();
    {
        const uint32_t* a = reinterpret_cast<const uint32_t*>(&env);
        uint32_t* b = reinterpret_cast<uint32_t*>(&s.env[g]);
        for (int i = l; i < (int)(sizeof(tz_state) / 4); i += 64) b[i] = a[i];
    }
    if (l == 0) {
        s.bank[g] = (uint8_t)dbank;
        s.alloc[g] = count;
    }
}

// ---- tz_search_step_wide: step_kernel's copy, one level of the kept subtree per launch, over the whole device --------------
// step_kernel lays the kept subtree out in plain breadth-first order: level L is a contiguous range [lo, hi) of the destination and
// level L + 1 is the children of level L in parent order, starting at hi.  So a level is an exclusive scan of the parents' nchild
// (block scan, scan of the block sums, offsets applied by the readers) and one thread per child; the level boundary is the
// kernel boundary and the host reads the level's total to size the next launches.  Every byte written is what step_kernel writes.

// Everything of step_kernel but the copy below the new root, for every game: status[g] = 1 iff a subtree is left to copy.
template <int N>
__global__ __launch_bounds__(64) void step_wide_root_kernel(SearchDev s, const uint16_t* actions, uint32_t* status) {
    const int g = blockIdx.x, l = lane_id();
    __shared__ tz_state env;
    const int sbank = s.bank[g], dbank = 1 - sbank;
    const size_t sb = slab_base(s, sbank, g), db = slab_base(s, dbank, g);
    if (s.t.eval_tag[sb] != TZ_EVAL_VALUE && s.t.eval_bits[sb] == 0) {  // root.is_terminal()
        if (l == 0) status[g] = 0;
        return;
    }
    const int action = actions[g];
    const int nc = s.t.nchild[sb];
    const uint32_t c0 = s.t.child0[sb];
    int found = -1;
    for (int i = l; i < nc; i += 64)
        if (s.t.action[sb + c0 + i] == action) found = i;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(found, d);
        found = o > found ? o : found;
    }
    if (l == 0) {
        if (found < 0) {
            write_default_node(s, db);
        } else {
            copy_node(s, db, sb + c0 + found);
            s.bfs_src[(size_t)g * s.cap] = c0 + (uint32_t)found;
        }
        status[g] = found < 0 ? 0 : 1;
    }
    load_state(&env, &s.env[g]);
    __syncthreads();
    apply_move<N>(&env, action);
    __syncthreads();
    {
        const uint32_t* a = reinterpret_cast<const uint32_t*>(&env);
        uint32_t* b = reinterpret_cast<uint32_t*>(&s.env[g]);
        for (int i = l; i < (int)(sizeof(tz_state) / 4); i += 64) b[i] = a[i];
    }
    if (l == 0) {
        s.bank[g] = (uint8_t)dbank;  // the level kernels below find the source in the other bank
        s.alloc[g] = 1;
    }
}

// Level [lo, lo + n) of game g's destination: off[i] = exclusive sum of nchild of the parents before parent i within its block of
// TZ_STEP_WIDE_BLOCK, sums[b] = block b's total.
__global__ __launch_bounds__(TZ_STEP_WIDE_BLOCK) void step_wide_scan_kernel(SearchDev s, StepWideDev w, int g, uint32_t lo, uint32_t n) {
    __shared__ int wave_total[TZ_STEP_WIDE_BLOCK / 64];
    const int t = threadIdx.x, l = lane_id(), wv = t >> 6;
    const uint32_t i = blockIdx.x * (uint32_t)TZ_STEP_WIDE_BLOCK + t;
    const size_t sb = slab_base(s, 1 - s.bank[g], g);
    const uint32_t* bsrc = s.bfs_src + (size_t)g * s.cap;
    const int cn = i < n ? (int)s.t.nchild[sb + bsrc[lo + i]] : 0;
    const int incl = wave_incl_scan(cn);
    if (l == 63) wave_total[wv] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < TZ_STEP_WIDE_BLOCK / 64; k++) {
        before += k < wv ? wave_total[k] : 0;
        total += wave_total[k];
    }
    if (i < n) w.off[i] = (uint32_t)(before + incl - cn);
    if (t == 0) w.sums[blockIdx.x] = (uint32_t)total;
}

// One wave turns the nb block sums into exclusive sums, TZ_STEP_WIDE_SUMS at a time with a carry, and leaves the level's total
// in *w.total (0 and the overflow flag when it would not fit; the destination has the source's capacity, so it fits).
__global__ __launch_bounds__(TZ_STEP_WIDE_SUMS) void step_wide_sums_kernel(SearchDev s, StepWideDev w, int g, uint32_t hi, uint32_t nb) {
    const int l = lane_id();
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += TZ_STEP_WIDE_SUMS) {
        const uint32_t b = b0 + l;
        const int v = b < nb ? (int)w.sums[b] : 0;
        const int incl = wave_incl_scan(v);
        if (b < nb) w.sums[b] = carry + (uint32_t)(incl - v);
        carry += (uint32_t)__shfl(incl, 63);
    }
    if (l == 0) {
        if (hi + carry > (uint32_t)s.cap) {
            atomicMax(s.error_flag, 1);
            carry = 0;
        }
        *w.total = carry;
        s.alloc[g] = hi + carry;
    }
}

// One thread per child c of the level's `total`: its parent is the last i with offset(i) <= c, found in the block sums and then
// in the block's offsets; thread i < n also writes child0 of parent i.
__global__ __launch_bounds__(256) void step_wide_copy_kernel(SearchDev s, StepWideDev w, int g, uint32_t lo, uint32_t n, uint32_t total) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    const int dbank = s.bank[g];
    const size_t sb = slab_base(s, 1 - dbank, g), db = slab_base(s, dbank, g);
    uint32_t* bsrc = s.bfs_src + (size_t)g * s.cap;
    const uint32_t hi = lo + n;
    if (c < n) {
        const uint32_t src = bsrc[lo + c];
        if (s.t.nchild[sb + src]) s.t.child0[db + lo + c] = hi + w.sums[c / TZ_STEP_WIDE_BLOCK] + w.off[c];
    }
    if (c >= total) return;
    const uint32_t nb = (n + TZ_STEP_WIDE_BLOCK - 1) / TZ_STEP_WIDE_BLOCK;
    uint32_t a = 0, z = nb;  // sums[a] <= c < sums[z] (sums[nb] = total)
    while (z - a > 1) {
        const uint32_t m = (a + z) >> 1;
        if (w.sums[m] <= c) a = m; else z = m;
    }
    const uint32_t r = c - w.sums[a];
    const uint32_t first = a * TZ_STEP_WIDE_BLOCK;
    uint32_t p = first, q = first + TZ_STEP_WIDE_BLOCK < n ? first + TZ_STEP_WIDE_BLOCK : n;  // off[p] <= r < off[q]
    while (q - p > 1) {
        const uint32_t m = (p + q) >> 1;
        if (w.off[m] <= r) p = m; else q = m;
    }
    const uint32_t k = r - w.off[p];
    const uint32_t from = s.t.child0[sb + bsrc[lo + p]] + k;
    copy_node(s, db + hi + c, sb + from);
    bsrc[hi + c] = from;
}

// restart_terminal_envs, batched.rs:185-203 (and BatchedMCTS::new when force_all)
template <int N>
__global__ __launch_bounds__(64) void restart_kernel(SearchDev s, const int32_t* choice, int8_t* terminal_out, int force_all,
                                                     int with_moves) {
    const int g = blockIdx.x, l = lane_id();
    __shared__ tz_state env;
    load_state(&env, &s.env[g]);
    __syncthreads();
    int why = 0;
    const int t = force_all ? TZ_TERMINAL_NONE : terminal<N>(&env, &why);
    if (l != 0) return;
    if (terminal_out) terminal_out[g] = (int8_t)t;
    s.term_reason[g] = (int8_t)why;
    // winner colour: the terminal is from the side to move
    s.term_winner[g] = (uint8_t)(t == TZ_TERMINAL_DRAW ? 2 : t == TZ_TERMINAL_WIN ? env.to_move : 1 - env.to_move);
    if (t == TZ_TERMINAL_NONE && !force_all) return;
    write_opening<N>(&s.env[g], s.half_komi, choice ? choice[g] : 0, with_moves != 0);
    write_default_node(s, slab_base(s, s.bank[g], g));
    s.alloc[g] = 1;
}

// Validated replay step (Replay::from_str re-validates every move, target.rs:248-268): applies actions[g] to
// game g's position iff it is one of its legal moves; ok[g] = 1 applied, 0 illegal (position unchanged),
// -1 position already terminal.  Trees are reset.  0xFFFF = no move for this game.
template <int N>
__global__ __launch_bounds__(64) void play_moves_kernel(SearchDev s, const uint16_t* actions, int8_t* ok) {
    constexpr int NN = N * N;
    const int g = blockIdx.x, l = lane_id();
    __shared__ tz_state env;
    __shared__ uint8_t reach[NN * 4];
    __shared__ uint16_t acts[1024];
    const int a = actions[g];
    if (a == 0xFFFF) {
        if (l == 0) ok[g] = 0;
        return;
    }
    load_state(&env, &s.env[g]);
    __syncthreads();
    if (terminal<N>(&env) != TZ_TERMINAL_NONE) {
        if (l == 0) ok[g] = -1;
        return;
    }
    // The row holds every move of a position up to 5x5 and of a 6x6 position within max_actions.  Of a wider 6x6 position
    // gen_moves writes the moves that fit and leaves the rest of the row as it is, hence "no move" in every entry first.  A move
    // that is not among the written ones of such a position cannot be judged: flag 3, position unchanged.
    for (int i = l; i < 1024; i += 64) acts[i] = 0xFFFF;
    const int n = gen_moves<N>(&env, reach, acts, 1024);
    bool hit = false;
    for (int i = l; i < n && i < 1024; i += 64) hit = hit || acts[i] == a;
    if (!__any(hit)) {
        if (l == 0) {
            ok[g] = 0;
            if (n > 1024) atomicMax(s.error_flag, 3);
        }
        return;
    }
    apply_move<N>(&env, a);
    __syncthreads();
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&env);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s.env[g]);
        for (int i = l; i < (int)(sizeof(tz_state) / 4); i += 64) dst[i] = src[i];
    }
    if (l == 0) {
        ok[g] = 1;
        write_default_node(s, slab_base(s, s.bank[g], g));
        s.alloc[g] = 1;
    }
}

// a wave-uniform 64-bit value held in scalar registers
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// Uniformly random legal play (Environment::new_opening_with_random_steps after the opening, env.rs:81-95): up to `steps` plies per
// game in one launch, the position in LDS throughout.  The draw of a ply is keyed by (seed, game, the position's own ply), so a
// playout made in two calls is the playout made in one.  key = tz_mix64(seed).  A game stops early when it has no legal move
// (env.rs:89-91), when its move list is wider than the row (flag 3, the position before that ply stays), or, with
// TZ_RANDOM_STOP_AT_TERMINAL, when it is over; without that flag terminal() is never asked, as in the reference.  Trees are reset.
// moves_out / nlegal_out are [batch][steps], 0xFFFF / 0 past played_out[g].
template <int N>
__global__ __launch_bounds__(64) void random_steps_kernel(SearchDev s, uint64_t key, uint64_t game_base, int steps, int stop_at_terminal,
                                                          uint16_t* moves_out, uint16_t* nlegal_out, int32_t* played_out) {
    constexpr int NN = N * N;
    const int g = blockIdx.x, l = lane_id();
    __shared__ tz_state env;
    __shared__ uint8_t reach[NN * 4];
    __shared__ uint16_t acts[1024];
    load_state(&env, &s.env[g]);
    __syncthreads();
    const uint64_t game_key = tz_mix64(key ^ (game_base + (uint64_t)g));   // blockIdx and kernel arguments: scalar
    uint16_t* mv = moves_out + (size_t)g * steps;
    uint16_t* nl = nlegal_out + (size_t)g * steps;
    int played = 0;
    for (; played < steps; played++) {
        if (stop_at_terminal && terminal<N>(&env) != TZ_TERMINAL_NONE) break;
        const int n = __builtin_amdgcn_readfirstlane(gen_moves<N>(&env, reach, acts, 1024));
        if (n == 0) break;
        if (n > 1024) {   // gen_moves cannot hand out the moves past the row
            if (l == 0) atomicMax(s.error_flag, 3);
            break;
        }
        const uint64_t ply = uniform64((uint64_t)env.ply);
        const uint64_t u = tz_mix64(game_key ^ ply);
        const int j = (int)(((u >> 32) * (uint64_t)n) >> 32);   // < n: (u >> 32) < 2^32
        const int a = __builtin_amdgcn_readfirstlane((int)acts[j]);
        if (l == 0) {
            mv[played] = (uint16_t)a;
            nl[played] = (uint16_t)n;
        }
        apply_move<N>(&env, a);
        __syncthreads();
    }
    for (int i = played + l; i < steps; i += 64) {
        mv[i] = 0xFFFF;
        nl[i] = 0;
    }
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&env);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&s.env[g]);
        for (int i = l; i < (int)(sizeof(tz_state) / 4); i += 64) dst[i] = src[i];
    }
    if (l == 0) {
        played_out[g] = played;
        write_default_node(s, slab_base(s, s.bank[g], g));
        s.alloc[g] = 1;
    }
}

__global__ void reset_games_kernel(SearchDev s, const int32_t* idx, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int g = idx[i];
    write_default_node(s, slab_base(s, s.bank[g], g));
    s.alloc[g] = 1;
}

// gumbel: start_node[g] = index of the chosen root child (child_index modulo handled by host)
__global__ void set_start_kernel(SearchDev s, const int32_t* child_index) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.batch) return;
    const size_t base = slab_base(s, s.bank[g], g);
    s.start_node[g] = (int32_t)(s.t.child0[base] + (uint32_t)child_index[g]);
}

// recompute root statistics after sequential halving, batched.rs:373-406
__global__ __launch_bounds__(64) void gumbel_fixup_kernel(SearchDev s) {
    const int g = blockIdx.x, l = lane_id();
    const size_t base = slab_base(s, s.bank[g], g);
    const int nc = s.t.nchild[base];
    const uint32_t c0 = s.t.child0[base];
    if (nc == 0) return;
    uint32_t sum = 0;
    bool any_loss = false;
    for (int i = l; i < nc; i += 64) {
        sum += s.t.visits[base + c0 + i];
        any_loss = any_loss || s.t.eval_tag[base + c0 + i] == TZ_EVAL_LOSS;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d);
    Ev mn;
    bool all_known;
    children_min_allknown(s, base, c0, nc, 0xFFFFFFFFu, Ev{0, 0}, mn, all_known);
    Ev ev;
    if (__any(any_loss) || all_known) {
        ev = ev_negate(mn);
    } else {
        float sp = 0.0f, wq = 0.0f;  // sequential sums in child order
        for (int i = 0; i < nc; i++)
            if (s.t.visits[base + c0 + i] > 0) sp = sp + s.t.prob[base + c0 + i];
        for (int i = 0; i < nc; i++)
            if (s.t.visits[base + c0 + i] > 0) {
                const Ev ce{s.t.eval_tag[base + c0 + i], s.t.eval_bits[base + c0 + i]};
                wq = wq + s.t.prob[base + c0 + i] * ev_to_f32(ev_negate(ce));
            }
        ev = ev_value(wq / sp);
    }
    if (l == 0) {
        s.t.visits[base] = sum + 1;
        s.t.eval_tag[base] = (uint8_t)ev.tag;
        s.t.eval_bits[base] = ev.bits;
        if (ev_known(ev)) s.t.std_dev[base] = 0.0f;
    }
}

}  // namespace

#define TZ_DISPATCH_N(n, CALL)                     \
    switch (n) {                                   \
        case 3: { constexpr int NB = 3; CALL; } break; \
        case 4: { constexpr int NB = 4; CALL; } break; \
        case 5: { constexpr int NB = 5; CALL; } break; \
        case 6: { constexpr int NB = 6; CALL; } break; \
        default: return tz_fail(TZ_EINVAL, "unsupported board size"); \
    }

// the instantiation of the walk for SearchDev::select_rule; used inside TZ_DISPATCH_N
#define TZ_DISPATCH_RULE(rule, CALL)                                              \
    switch (rule) {                                                               \
        case TZ_SELECT_PUCT: { constexpr int RB = TZ_SELECT_PUCT; CALL; } break;   \
        case TZ_SELECT_UCT: { constexpr int RB = TZ_SELECT_UCT; CALL; } break;     \
        case TZ_SELECT_IMPROVED: { constexpr int RB = TZ_SELECT_IMPROVED; CALL; } break; \
        default: return tz_fail(TZ_EINVAL, "unknown selection rule");             \
    }

// diagnostic: the f32 primitives the tree kernels rely on being bit-identical with the host
__global__ void device_math_kernel(int op, const float* a, const float* b, float* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (op) {
        case 0: out[i] = tz_expf(a[i]); break;
        case 1: out[i] = tz_logf(a[i]); break;
        case 2: out[i] = sqrtf(a[i]); break;
        case 3: out[i] = a[i] / b[i]; break;
        case 4: out[i] = tz_powif(TZ_DISCOUNT, (int)a[i]); break;
        default: out[i] = (a[i] + b[i]) * a[i]; break;
    }
}

#define TZ_LAUNCH_CHECK()                                                                       \
    do {                                                                                        \
        hipError_t _e = hipGetLastError();                                                      \
        if (_e != hipSuccess) return tz_fail(TZ_EDEVICE, std::string("kernel launch: ") + hipGetErrorString(_e)); \
    } while (0)

extern "C" int tz_device_math(int op, const float* a, const float* b, float* out, int n) {
    if (!a || !b || !out || n <= 0) return tz_fail(TZ_EINVAL, "tz_device_math: bad argument");
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    TZ_HIP(hipMalloc(&da, n * 4));
    TZ_HIP(hipMalloc(&db, n * 4));
    TZ_HIP(hipMalloc(&dout, n * 4));
    TZ_HIP(hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice));
    TZ_HIP(hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice));
    device_math_kernel<<<(n + 255) / 256, 256>>>(op, da, db, dout, n);
    TZ_HIP(hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    return TZ_OK;
}

int tz_tree_descend(const SearchDev& s, bool from_start_nodes, hipStream_t st) {
    TZ_DISPATCH_N(s.n, TZ_DISPATCH_RULE(s.select_rule, (descend_kernel<NB, RB><<<s.batch, 64, 0, st>>>(s, from_start_nodes ? 1 : 0))));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_compact_leaves(const SearchDev& s, hipStream_t st) {
    compact_kernel<<<1, 1024, 0, st>>>(s);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_expand(const SearchDev& s, const NetOut& out, hipStream_t st) {
    const size_t smem = 2 * TZ_MAX_DEPTH * sizeof(uint32_t) + 2 * (size_t)s.max_actions * sizeof(float);
    TZ_DISPATCH_N(s.n, (expand_kernel<NB><<<s.batch, 64, smem, st>>>(s, out)));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_apply_noise(const SearchDev& s, const float* noise_dev, int amax, float ratio, hipStream_t st) {
    noise_kernel<<<s.batch, 64, 0, st>>>(s, noise_dev, amax, ratio);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_root_info(const SearchDev& s, tz_root_info* out_dev, hipStream_t st) {
    TZ_DISPATCH_N(s.n, (root_info_kernel<NB><<<s.batch, 64, 0, st>>>(s, out_dev)));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_root_children(const SearchDev& s, int amax, uint16_t* move_idx, uint32_t* visits, uint8_t* eval_tag,
                          uint32_t* eval_bits, float* logit, float* prob, float* std_dev, hipStream_t st) {
    root_children_kernel<<<s.batch, 64, 0, st>>>(s, amax, move_idx, visits, eval_tag, eval_bits, logit, prob, std_dev);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_node(const SearchDev& s, int game, const uint16_t* path_dev, int len, uint32_t* out_words, int* status, int amax,
                 uint16_t* move_idx, uint32_t* visits, uint8_t* eval_tag, uint32_t* eval_bits, float* logit, float* prob, float* std_dev,
                 hipStream_t st) {
    node_kernel<<<1, 64, 0, st>>>(s, game, path_dev, len, out_words, status, amax, move_idx, visits, eval_tag, eval_bits, logit, prob, std_dev);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_select_best(const SearchDev& s, uint16_t* out_dev, hipStream_t st) {
    select_best_kernel<<<s.batch, 64, 0, st>>>(s, out_dev);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_step(const SearchDev& s, const uint16_t* actions_dev, hipStream_t st) {
    TZ_DISPATCH_N(s.n, (step_kernel<NB><<<s.batch, 64, 0, st>>>(s, actions_dev)));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_step_wide_roots(const SearchDev& s, const uint16_t* actions_dev, uint32_t* status_dev, hipStream_t st) {
    TZ_DISPATCH_N(s.n, (step_wide_root_kernel<NB><<<s.batch, 64, 0, st>>>(s, actions_dev, status_dev)));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_step_wide_scan(const SearchDev& s, const StepWideDev& w, int game, uint32_t lo, uint32_t n, hipStream_t st) {
    const uint32_t nb = (n + TZ_STEP_WIDE_BLOCK - 1) / TZ_STEP_WIDE_BLOCK;
    step_wide_scan_kernel<<<nb, TZ_STEP_WIDE_BLOCK, 0, st>>>(s, w, game, lo, n);
    TZ_LAUNCH_CHECK();
    step_wide_sums_kernel<<<1, TZ_STEP_WIDE_SUMS, 0, st>>>(s, w, game, lo + n, nb);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_step_wide_copy(const SearchDev& s, const StepWideDev& w, int game, uint32_t lo, uint32_t n, uint32_t total, hipStream_t st) {
    const uint32_t threads = n > total ? n : total;
    step_wide_copy_kernel<<<(threads + 255) / 256, 256, 0, st>>>(s, w, game, lo, n, total);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_restart(const SearchDev& s, const int32_t* choice_dev, int8_t* terminal_dev, bool force_all,
                    bool with_opening_moves, hipStream_t st) {
    TZ_DISPATCH_N(s.n, (restart_kernel<NB><<<s.batch, 64, 0, st>>>(s, choice_dev, terminal_dev, force_all ? 1 : 0,
                                                                  with_opening_moves ? 1 : 0)));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_play_moves(const SearchDev& s, const uint16_t* actions_dev, int8_t* ok_dev, hipStream_t st) {
    TZ_DISPATCH_N(s.n, (play_moves_kernel<NB><<<s.batch, 64, 0, st>>>(s, actions_dev, ok_dev)));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_random_steps(const SearchDev& s, uint64_t seed, uint64_t game_base, int steps, bool stop_at_terminal, uint16_t* moves_dev,
                         uint16_t* nlegal_dev, int32_t* played_dev, hipStream_t st) {
    const uint64_t key = tz_mix64(seed);
    TZ_DISPATCH_N(s.n, (random_steps_kernel<NB><<<s.batch, 64, 0, st>>>(s, key, game_base, steps, stop_at_terminal ? 1 : 0, moves_dev,
                                                                        nlegal_dev, played_dev)));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_reset_games(const SearchDev& s, const int32_t* idx_dev, int count, hipStream_t st) {
    if (count <= 0) return TZ_OK;
    reset_games_kernel<<<(count + 255) / 256, 256, 0, st>>>(s, idx_dev, count);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_set_start_children(const SearchDev& s, const int32_t* child_index_dev, hipStream_t st) {
    set_start_kernel<<<(s.batch + 255) / 256, 256, 0, st>>>(s, child_index_dev);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_gumbel_root_fixup(const SearchDev& s, hipStream_t st) {
    gumbel_fixup_kernel<<<s.batch, 64, 0, st>>>(s);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_principal_variation(const SearchDev& s, int game, uint16_t* moves_dev, int cap, int* len_dev, hipStream_t st) {
    principal_variation_kernel<<<1, 64, 0, st>>>(s, game, moves_dev, cap, len_dev);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_descend_batch(const SearchDev& s, const LeafBatchDev& b, hipStream_t st) {
    TZ_DISPATCH_N(s.n, TZ_DISPATCH_RULE(s.select_rule, (descend_batch_kernel<NB, RB><<<s.batch, 64, 0, st>>>(s, b))));
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_compact_batch(const SearchDev& s, const LeafBatchDev& b, hipStream_t st) {
    compact_batch_kernel<<<1, 1024, 0, st>>>(s, b);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
int tz_tree_expand_batch(const SearchDev& s, const LeafBatchDev& b, const NetOut& out, hipStream_t st) {
    const size_t smem = 2 * (size_t)s.max_actions * sizeof(float);
    TZ_DISPATCH_N(s.n, (leaf_policy_kernel<NB><<<s.batch * b.leaves, 64, smem, st>>>(s, b, out)));
    TZ_LAUNCH_CHECK();
    expand_batch_kernel<<<s.batch, 64, 0, st>>>(s, b);
    TZ_LAUNCH_CHECK();
    return TZ_OK;
}
