/*
 * takzero_hip.h — C ABI of libtakzero_hip.so, the MI355X (gfx950) engine for the
 * takzero self-play / reanalyze hot path (batched MCTS + policy/value net forward).
 *
 * The reference (ViliamVadocz/takzero) has no FFI of its own for this path: its seams are
 * the Rust traits `Agent` (takzero/src/search/agent.rs:5-14), `Network`
 * (takzero/src/network/mod.rs:10-45) and the struct `BatchedMCTS`
 * (takzero/src/search/node/batched.rs:24-409).  Every entry point below names the
 * reference item it replaces.  A Rust adapter maps these calls back
 * onto the reference's types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative TZ_E* code otherwise; the message
 *     is available from tz_last_error() (thread local).
 *   - caller owns every host buffer; the library owns device memory behind the handles.
 *   - one handle is driven from one host thread (the reference is single threaded,
 *     batched.rs:21-22); calls block until results are on the host unless noted.
 *   - randomness never crosses the ABI: Dirichlet / Gumbel / opening choices are inputs
 *     (the reference threads one StdRng through its calls; keeping the draws on the
 *     caller side is the only way an adapter can reproduce its stream).
 *   - moves are identified by the reference's policy index `move_index`
 *     (takzero/src/network/repr.rs:49-71): channel * N*N + row * N + column.
 *   - squares are indexed  sq = row * N + column  (row = rank-1, column = file).
 */
#ifndef TAKZERO_HIP_H
#define TAKZERO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TZ_MAX_N 6
#define TZ_MAX_SQUARES 36
/* upper bound on legal moves in one position for board sizes 3..5 (rows of 512); a 6x6 handle uses 1024: ask
 * tz_search_shape for the row width of a given handle */
#define TZ_MAX_ACTIONS 512
#define TZ_MAX_ACTIONS_6 1024

/* error codes */
#define TZ_OK 0
#define TZ_EINVAL (-1)   /* bad argument (size, index, null)                           */
#define TZ_EPARSE (-2)   /* malformed TPS / PTN / weight file                          */
#define TZ_EDEVICE (-3)  /* HIP runtime failure (message carries hipGetErrorString)    */
#define TZ_ENOMEM (-4)   /* host or device allocation failed                           */
#define TZ_ECAPACITY (-5)/* a per-game node pool or trajectory buffer overflowed, or a  */
                         /* position has more legal moves than max_actions             */
#define TZ_ESTATE (-6)   /* call not valid in the current state (e.g. noise on an      */
                         /* un-expanded root — batched.rs / noise.rs:12-15 assert)     */
#define TZ_ENUMERIC (-7) /* NaN produced by the net (reference panics: net5.rs:263)    */

/* piece type of the top of a stack */
#define TZ_EMPTY 0
#define TZ_FLAT 1
#define TZ_WALL 2
#define TZ_CAP 3

/* Eval tags, takzero/src/search/eval.rs:8-13 */
#define TZ_EVAL_VALUE 0
#define TZ_EVAL_WIN 1
#define TZ_EVAL_LOSS 2
#define TZ_EVAL_DRAW 3

/* Terminal, takzero/src/search/env.rs:27-31 (from the side to move) */
#define TZ_TERMINAL_NONE (-1)
#define TZ_TERMINAL_WIN 0
#define TZ_TERMINAL_LOSS 1
#define TZ_TERMINAL_DRAW 2

/*
 * Packed game state = the fields of fast_tak::Game<N,HALF_KOMI> that the reference reads
 * (repr.rs:169-228, env.rs:39-63).  Plain data, 376 bytes.
 */
typedef struct tz_state {
    uint64_t colors[TZ_MAX_SQUARES]; /* bit i = colour of the i-th piece from the bottom (0 white, 1 black) */
    uint8_t height[TZ_MAX_SQUARES];  /* number of pieces on the square                                     */
    uint8_t top[TZ_MAX_SQUARES];     /* TZ_EMPTY / TZ_FLAT / TZ_WALL / TZ_CAP                               */
    uint8_t stones[2];               /* remaining stones  [white, black]                                    */
    uint8_t caps[2];                 /* remaining capstones [white, black]                                  */
    uint8_t to_move;                 /* 0 white, 1 black                                                    */
    uint8_t n;                       /* board size 3..6                                                     */
    int8_t half_komi;                /* komi for black in half points (net5.rs:18 uses 4)                   */
    uint8_t pad0;
    uint16_t ply;
    uint16_t reversible_plies;
} tz_state;

typedef struct tz_net tz_net;       /* opaque: a network on one GPU  (Network + Agent impl)   */
typedef struct tz_search tz_search; /* opaque: BatchedMCTS<B, Game<N,HALF_KOMI>> on one GPU   */

/* architectures (takzero/src/network/{net4_simhash,net5,net6_simhash,net4_lcghash,net4_ensemble,net4_rnd}.rs) */
#define TZ_ARCH_NET4_SIMHASH 4
#define TZ_ARCH_NET5 5
#define TZ_ARCH_NET6_SIMHASH 6
/* the trunk, heads and 2^32-bit set of net4_simhash; the set's index is an integer hash of planes * lcghash_init
 * (net4_lcghash.rs:202-242).  4x4 only.  Everything said about SimHash nets below holds for it. */
#define TZ_ARCH_NET4_LCGHASH 14
/* the trunk and heads of net4_simhash plus sixteen more value heads (`ensemble head i.*`); the local uncertainty is the population
 * variance of their values (net4_ensemble.rs:146-171, 225-233).  4x4 only; no set of seen positions, no RND. */
#define TZ_ARCH_NET4_ENSEMBLE 24
#define TZ_ENSEMBLE_SIZE 16
/* the trunk and heads of net4_simhash plus two conv towers, `rnd_predictor.*` and `rnd_target.*` (LayerNorm([28,4,4]), conv 28->32,
 * four 32-filter residual blocks, a last conv + BatchNorm, 512 outputs), and the `min` / `max` of their normalisation; the local
 * uncertainty is clamp((sum_512 (predictor - target)^2 - min) / (max - min), 0, 1) * 4 (net4_rnd.rs:126-166, 210-230).  4x4 only; no
 * set of seen positions; tz_trainer_rnd4_enable trains the predictor in the step (tz_trainer_rnd_enable stays net5's). */
#define TZ_ARCH_NET4_RND 34
/* test architecture: same graph as net5 on any board size with configurable depth, no RND/hash */
#define TZ_ARCH_TEST 100

/* arithmetic of the trunk */
#define TZ_PREC_BF16 0 /* NHWC bf16 activations/weights, fp32 accumulate on MFMA: 5 % faster, logits 1e-3..7e-3 off fp32 */
#define TZ_PREC_F32 1  /* fp32 everywhere on plain FMA kernels (validation path)                          */
#define TZ_PREC_F16 2  /* the throughput default: the same MFMA kernels with IEEE fp16 storage (saturating), fp32
                          accumulate: logits within ~2e-4 relative of fp32 (1.5e-4 absolute at random-init scale) */
#define TZ_PREC_F16X2 3 /* split precision: every operand a hi/lo pair of halves (22-bit significand), three fp16 MFMAs
                          per product with fp32 accumulate: logits within 1e-3 absolute of the fp32 LibTorch graph at
                          trained logit scale (|logit| ~ 10), the north star's tolerance; ~3x the MFMA work */
#define TZ_PREC_F16C8 4 /* fp16 products with FP8 corrections: the main product wh*xh as in TZ_PREC_F16, the two correction
                          products wl*xh + wh*xl of the split form on OCP FP8 (E4M3) copies of the operands through
                          v_mfma_f32_16x16x128_f8f6f4 (twice the fp16 rate): a correction only has to be good to a few
                          bits.  Logits within 1e-3 absolute at trained logit scale like TZ_PREC_F16X2 (about 30x
                          closer to fp32 than TZ_PREC_F16), ~2x the MFMA time of TZ_PREC_F16 instead of 3x */
#define TZ_PREC_F16C6 5 /* the same with the corrections on FP6 (E2M3) copies and one power-of-two scale per block of 32 input
                          channels, through v_mfma_scale_f32_16x16x128_f8f6f4 at four times the fp16 rate (round 3): 1.5x the
                          MFMA time of TZ_PREC_F16, 8 boards per workgroup like it, the same logit error as TZ_PREC_F16C8.
                          5x5 and 6x6 networks. */

/* built-in agents for tz_search_create (takzero/src/search/agent.rs:16-87) */
#define TZ_AGENT_NET 0
#define TZ_AGENT_DUMMY 1
#define TZ_AGENT_SIMPLE 2

const char* tz_last_error(void);
int tz_version(void);
int tz_device_count(void);

/* ---------- text / index helpers (fast-tak / takparse formats) ---------- */
int tz_state_from_tps(const char* tps, int n, int half_komi, tz_state* out);
int tz_state_to_tps(const tz_state* s, char* buf, int buflen);
int tz_move_to_ptn(int n, uint16_t move_index, char* buf, int buflen);
int tz_move_from_ptn(int n, const char* ptn, uint16_t* move_index_out);
/* number of policy logits for board size n: output_size::<N>(), repr.rs:119-121 */
int tz_policy_size(int n);
/* number of input planes: input_channels::<N>(), repr.rs:137-142 */
int tz_input_channels(int n);

/* ---------- Network lifecycle: Network::{new, save, load, load_partial, clone}  (network/mod.rs:10-45) ---------- */
/* blocks = number of residual blocks for TZ_ARCH_TEST (ignored otherwise). */
int tz_net_create(int board_n, int arch, int device_id, int precision, int blocks, tz_net** out);
/* Network::new(device, seed) (network/mod.rs:11; net5.rs:152-170): tch's default initialisers, draws from a generator
 * keyed by (seed, variable name); the net is usable afterwards. */
int tz_net_init_random(tz_net* net, uint64_t seed);
/* Network::load (network/mod.rs:24-28; net6_simhash.rs:173-190).  The file is recognised by its content: a LibTorch
 * archive as tch's VarStore::save writes it (`model_latest.ot`, `model_NNNNNNN.ot`: read natively, no LibTorch needed) or
 * the flat .tzw container of takzero_amd.weights (named fp32 tensors).  SimHash nets also pick up `bitvec.bin` from the
 * same directory when it is there.  A failed load leaves the previous weights active (selfplay/src/main.rs:112-115). */
int tz_net_load_weights(tz_net* net, const char* path);
/* The same load in two halves, for a host that does not want to stop playing while a new model_latest.ot is read (selfplay's
 * hot reload, selfplay/src/main.rs:107-120).  tz_net_load_prepare parses the file and builds the device weights in fresh buffers;
 * it touches nothing of the live network and may run on another thread while `net` is evaluating.  tz_net_load_commit puts them
 * in place (a device synchronisation and a pointer swap; for a SimHash net also the bitvec.bin beside the file) and must be
 * called where tz_net_load_weights could be: not concurrently with a forward of `net`.  A failed prepare leaves nothing behind;
 * prepared weights that are not wanted any more go to tz_net_load_discard. */
typedef struct tz_pending_weights tz_pending_weights;
int tz_net_load_prepare(tz_net* net, const char* path, tz_pending_weights** out);
int tz_net_load_commit(tz_net* net, tz_pending_weights* pending);
int tz_net_load_discard(tz_pending_weights* pending);
int tz_net_load_weights_mem(tz_net* net, const void* data, size_t bytes);
/* Network::load_partial (network/mod.rs:30-35): variables the file does not hold (or holds with another size) keep their
 * values; their names come back newline-separated in missing_out (may be NULL), their number in n_missing_out. */
int tz_net_load_partial(tz_net* net, const char* path, char* missing_out, int missing_cap, int* n_missing_out);
/* Network::save (network/mod.rs:16-18; net6_simhash.rs:152-170): `*.tzw` = the flat container, anything else = a LibTorch
 * archive with tch's variable names, written to `<path>.part` and renamed; SimHash nets write `bitvec.bin` beside it. */
int tz_net_save(tz_net* net, const char* path);
/* Network::clone(device) (network/mod.rs:37-44): the same variables (and SimHash set) on another GPU. */
int tz_net_clone(tz_net* net, int device_id, tz_net** out);
/* One variable of the host-side VarStore by name (`.a.` / `.b.` for the two SmallBlocks of a block); out may be NULL to
 * ask for the element count only. */
int tz_net_get_tensor(tz_net* net, const char* name, float* out, uint64_t count, uint64_t* count_out);
/* enumeration of that store, in name order (as tz_trainer_tensor_count / _info) */
int tz_net_tensor_count(tz_net* net);
int tz_net_tensor_info(tz_net* net, int i, char* name_out, int name_cap, uint64_t* count_out);
/* Converts a model file between the two containers (by content on the way in, by extension on the way out). */
int tz_weights_convert(const char* src, const char* dst);
int tz_net_destroy(tz_net* net);

/*
 * Agent::policy_value_uncertainty  (agent.rs:5-14; net5.rs:220-285)
 *   states[batch]; legal_idx[batch][amax] = move_index of each legal action in the caller's
 *   order, legal_count[batch] <= amax.
 *   logits_out[batch][amax]: raw logits of exactly those actions in that order (entries past
 *   legal_count are 0); value_out[batch] in [-1,1] from the side to move;
 *   variance_out[batch] in [0,4].  batch == 0 is TZ_EINVAL (net5.rs:226-227 asserts).
 */
int tz_net_eval(tz_net* net, int batch, const tz_state* states, const uint16_t* legal_idx,
                const int32_t* legal_count, int amax, float* logits_out, float* value_out,
                float* variance_out);
/* Debug path: the input planes game_repr writes (repr.rs:169-228), NCHW fp32,
 * planes_out[batch][channels*n*n], computed on the device by the same encoder. */
int tz_net_encode(tz_net* net, int batch, const tz_state* states, float* planes_out);
/* Full policy tensor [batch][policy_size] in the reference's NCHW flattening (net5.rs:238). */
int tz_net_forward_raw(tz_net* net, int batch, const tz_state* states, float* policy_out,
                       float* value_out, float* ube_out);

/* EnsembleNetwork::forward_core_and_ensemble(xs, false) (net4_ensemble.rs:157-171): the sixteen head values of every position,
 * out[batch][16].  TZ_EINVAL unless the net is TZ_ARCH_NET4_ENSEMBLE. */
int tz_net_ensemble_values(tz_net* net, int batch, const tz_state* states, float* out);

/* RndNetwork::forward_rnd(xs, false) (net4_rnd.rs:210-223): raw_out[batch] = sum_512 (predictor - target)^2, the values the
 * variance of tz_net_eval is made of (variance = clamp(max(e^ube, clamp((raw - min) / (max - min), 0, 1) * 4), 0, 4)) and what
 * update_rnd_normalization is fed with.  The same bits for a position wherever it sits in a batch, at every batch size and in every
 * precision but TZ_PREC_F32.  TZ_EINVAL unless the net is TZ_ARCH_NET4_RND. */
int tz_net_rnd_raw(tz_net* net, int batch, const tz_state* states, float* raw_out);

/* Hash nets (net4_simhash / net6_simhash / net4_lcghash): HashNetwork::get_indices / update_counts
 * (net6_simhash.rs:202-243, net4_lcghash.rs:202-249) and the bitvec.bin file that accompanies a model (net6_simhash.rs:152-190). */
int tz_net_hash_indices(tz_net* net, int batch, const tz_state* states, uint32_t* indices_out, int update);
int tz_net_load_bitset(tz_net* net, const char* path);
int tz_net_save_bitset(tz_net* net, const char* path);
/* HashNetwork::forward_hash for host states: seen_out[i] = 1 if position i's index is in the set, 0 if not; the set is not updated
 * (tz_search_hash_seen is the same on a search handle's positions).  TZ_EINVAL unless the net is a loaded hash net. */
int tz_net_hash_seen(tz_net* net, int batch, const tz_state* states, uint8_t* seen_out);

/* ---------- BatchedMCTS (search/node/batched.rs:32-409) ---------- */
/* BatchedMCTS::from_envs with default (empty-board) envs; node_capacity = node slots per game
 * (0 = default).  net may be NULL when agent_kind != TZ_AGENT_NET. */
int tz_search_create(tz_net* net, int agent_kind, int batch, int board_n, int half_komi,
                     int node_capacity, tz_search** out);
int tz_search_destroy(tz_search* s);
/* BATCH_SIZE, N, HALF_KOMI of the handle and the widest child list it can hold.
 *
 * max_actions is 64 on 3x3, 192 on 4x4, 512 on 5x5 and 1024 on 6x6.  The reference's child lists are Vecs and have no limit;
 * positions with more legal moves exist on every board size (tall stacks under the mover's control; none is near the games the
 * reference plays).  The Agent surface, tz_net_eval, takes its own amax and evaluates such positions like any other.  A search
 * handle does this with them:
 *   - tz_search_set_positions accepts any position: it generates no moves.
 *   - When a simulation reaches a node with more than max_actions legal moves, at the root or below it, that node is not
 *     expanded and gets no children, then or later; nothing is written past a row, and tz_search_pool_overflows does not count it.
 *     The visits along the path to it are counted without a backup, so the tree of that game is worth nothing from then on.
 *   - tz_search_simulate and tz_search_simulate_batch still run all their simulations or rounds and then return TZ_ECAPACITY
 *     with a text that names max_actions; every other game of the batch is exactly what it would be had the call succeeded.
 *     The report clears the condition, and each later call that reaches such a node reports it again.
 *   - tz_search_gumbel_sh returns the same error at its first simulation (an over-wide root) or at the end of the halving step in
 *     which a node below the root was reached; it selects nothing, and the trees keep the simulations made until then.
 *   - tz_search_set_positions over the game in question puts the handle back: from there it behaves like a fresh handle with the
 *     same history, with or without captured graphs.  After the error from tz_search_gumbel_sh, set every game again before the
 *     halving is repeated (the other games are part of the way through it). */
int tz_search_shape(tz_search* s, int* batch_out, int* board_n_out, int* half_komi_out, int* max_actions_out);
/* nodes_and_envs_mut: overwrite envs and reset their trees (reanalyze/src/main.rs:159-165). */
int tz_search_set_positions(tz_search* s, int count, const int32_t* game_idx, const tz_state* states);
int tz_search_get_positions(tz_search* s, tz_state* states_out /*[batch]*/);
/* BatchedMCTS::new openings: env.rs:65-79.  opening_choice[g] in [0,16): symmetry*2 + opposite. */
int tz_search_new_openings(tz_search* s, const int32_t* opening_choice);
/* BatchedMCTS::simulate called n_sims times (batched.rs:63-128); betas[batch]. Asynchronous
 * on the handle's stream; any later call that returns data synchronises.  TZ_ECAPACITY "more legal moves than max_actions":
 * see tz_search_shape. */
int tz_search_simulate(tz_search* s, const float* betas, int n_sims);
/* Node::simulate_batch (mcts.rs:268-328) applied to every root of the handle, `rounds` times: the search of the reference's tei and
 * analysis binaries (tei/src/main.rs:253, analysis/src/main.rs:35,78), which fills a network batch from one tree.  Per tree and
 * round: up to 4*leaves forwards (mcts.rs:281); Known results are backed up at once (:284); the loop ends when `leaves` leaves
 * need the network (:297).  One network call covers all trees' leaves.  backward_network_eval then runs per tree in collection
 * order (:307-327); a leaf collected more than once in a round is evaluated each time and its children are replaced each time
 * (mcts.rs:199-217), as in the reference.  betas[batch].  Asynchronous like tz_search_simulate.
 * tz_search_counters: simulations grow by the forwards actually made, nn_leaf_evals by the leaves sent to the network.
 * TZ_EINVAL: leaves < 1, rounds < 0, a null pointer, or batch * leaves > TZ_SIMULATE_BATCH_MAX_SLOTS.  Scratch for batch * leaves
 * leaf slots is allocated at the first call and grown on demand.  A full node pool behaves as in tz_search_simulate
 * (tz_search_pool_overflows).  The virtual_visits counter of the reference's `virtual` feature is not kept: selection does not
 * read it (the code that would is commented out, node/mod.rs:115-122) and it is back at zero after every call. */
#define TZ_SIMULATE_BATCH_MAX_SLOTS 16384
int tz_search_simulate_batch(tz_search* s, const float* betas, int leaves, int rounds);
/* The in-tree selection rule of Node::forward (mcts.rs:107-138).  The reference picks one by editing mcts.rs:132; here it is a
 * switch on the handle, read by tz_search_simulate, tz_search_simulate_batch, tz_search_gumbel_sh (below the sampled root child;
 * halving at the root is unchanged) and every native driver that runs on the handle (tz_selfplay_*, tz_reanalyze_*, tz_compete,
 * tz_puzzle_benchmark).  All three rules skip a winning child unless the parent is a proven loss, and break ties towards the
 * last child (Iterator::max_by_key). */
#define TZ_SELECT_PUCT 0     /* select_with_puct, policy.rs:78-95 with :140-156; the default */
#define TZ_SELECT_UCT 1      /* select_with_uct, policy.rs:104-117 with upper_confidence_bound :158-164: q + sqrt(ln N / n) +
                              * std_dev * beta.  An unvisited child scores +inf, so they are visited from the last to the first */
#define TZ_SELECT_IMPROVED 2 /* select_with_improved_policy, policy.rs:57-69 with improved_policy :36-48 and sigma_improve
                              * :131-138 (the non-root rule of Gumbel MuZero): softmax(completed q * sqrt(max visits) + logit) -
                              * n / (N + 1).  beta is not read */
/* Sets the rule.  Allowed at any time between calls: synchronises the handle's stream and drops its captured simulation graphs,
 * so the next simulations run (and are captured again) with the new rule.  TZ_EINVAL for an unknown rule; the rule then stays.
 * A NaN score (the reference's NotNan panics, policy.rs:113) surfaces as TZ_ENUMERIC from the simulate call.
 * With TZ_SELECT_IMPROVED and a full node pool (tz_search_pool_overflows), a leaf that was evaluated but not expanded counts as
 * needing initialisation, so its completed value is its parent's evaluation; the reference's trees have no such state. */
int tz_search_set_selection(tz_search* s, int rule);
int tz_search_get_selection(tz_search* s, int* rule_out);
/* Where the rounds of tz_search_simulate_batch spent their time since profiling was switched on (tz_search_profile with reset 1;
 * reset 1 or 2 also clears these): HIP-event time in ms of the forward kernel with the compaction, of the network call, and of
 * the backward pass with the leaf softmax, summed over `rounds` rounds.  Any pointer may be NULL. */
int tz_search_batch_profile(tz_search* s, double* forward_ms, double* net_ms, double* backward_ms, uint64_t* rounds);
/* Node::principal_variation (node/mod.rs:40-62, 87-90) of one root.  Follows select_best_action until a node needs
 * initialisation or is terminal.  moves_out[cap] receives move indices.  len_out receives the full length, even when it
 * exceeds cap. */
int tz_search_principal_variation(tz_search* s, int game, uint16_t* moves_out, int cap, int* len_out);
/* BatchedMCTS::apply_noise with caller-supplied Dirichlet samples (noise.rs:10-26):
 * noise[batch][amax], row g holds one sample of dimension n_children(g). */
int tz_search_apply_noise(tz_search* s, const float* noise, int amax, float ratio);
/* per-root summary: evaluation, visit_count, std_dev, number of children, terminal flag */
typedef struct tz_root_info {
    uint32_t visit_count;
    uint32_t n_children;
    uint8_t eval_tag;
    uint8_t is_terminal_env; /* env.terminal().is_some() */
    uint16_t ply;
    union { float value; uint32_t ply; } eval;
    float std_dev;
    float logit;
    float probability;
} tz_root_info;
int tz_search_root_info(tz_search* s, tz_root_info* out /*[batch]*/);
/* children of every root in fast-tak possible_moves order (callers zip by position:
 * selfplay/src/main.rs:249-253).  Arrays are [batch][amax]; any pointer may be NULL. */
int tz_search_root_children(tz_search* s, int amax, uint16_t* move_idx, uint32_t* visits,
                            uint8_t* eval_tag, uint32_t* eval_bits, float* logit, float* prob,
                            float* std_dev);
/* Below the root: the reference's Node.children is a public field (node/mod.rs:14-23) that puzzle and visualize_search read.
 * The node reached from game `game`'s root by the moves path[0..path_len) (move indices; path_len 0 = the root): node_out = its
 * statistics (ply = the root's ply + path_len; is_terminal_env = Node::is_terminal), children rows of width amax as in
 * tz_search_root_children (any pointer may be NULL).  TZ_EINVAL if the path leaves the tree. */
int tz_search_node(tz_search* s, int game, const uint16_t* path, int path_len, tz_root_info* node_out, int amax, uint16_t* move_idx,
                   uint32_t* visits, uint8_t* eval_tag, uint32_t* eval_bits, float* logit, float* prob, float* std_dev);
/* Node::select_best_action per root (node/mod.rs:132-161). 0xFFFF for roots without children. */
int tz_search_select_best_actions(tz_search* s, uint16_t* actions_out /*[batch]*/);
/* Node::improved_policy(visitations) per root (policy.rs:23-48), [batch][amax]. */
int tz_search_improved_policy(tz_search* s, float visitations, int amax, float* policy_out);
/* the same with one visitation count per game: reanalyze passes each root's most_visited_count()
 * (reanalyze/src/main.rs:196-202) */
int tz_search_improved_policy_each(tz_search* s, const float* visitations, int amax, float* policy_out);
/* Node::ube_target(beta) per root (node/mod.rs:215-230). */
int tz_search_ube_target(tz_search* s, float beta, float* out /*[batch]*/);
/* BatchedMCTS::step (batched.rs:131-144): descend (subtree reuse) + env.step; skipped for
 * terminal roots.  actions[batch] are move indices. */
int tz_search_step(tz_search* s, const uint16_t* actions);
/* tz_search_step for a tree of an engine's size.  tz_search_step copies a game's kept subtree with one wave, which suits
 * thousands of small trees; this call takes the games one after another and gives each the whole device: per level of the kept
 * subtree, a scan of the parents' child counts in blocks of TZ_STEP_WIDE_BLOCK, one wave that scans the block sums
 * TZ_STEP_WIDE_SUMS at a time, and one thread per child copied; the host reads the level's child count (4 bytes) to size the next
 * launches.  Everything a caller can observe is what tz_search_step leaves: trees (slot for slot), positions, pool usage,
 * counters, errors; the handle's captured simulation graphs stay valid.  Scratch of 4 bytes per node slot of one game is
 * allocated at the first call. */
#define TZ_STEP_WIDE_BLOCK 128
#define TZ_STEP_WIDE_SUMS 64
int tz_search_step_wide(tz_search* s, const uint16_t* actions);
/* BatchedMCTS::restart_terminal_envs (batched.rs:185-203): finished games get a fresh opening
 * (opening_choice as above) and a fresh tree; terminal_out[g] = TZ_TERMINAL_* of the game
 * that ended, TZ_TERMINAL_NONE otherwise. */
int tz_search_restart_terminal(tz_search* s, const int32_t* opening_choice, int8_t* terminal_out);
/* Details of the games that ended in the last tz_search_restart_terminal call: reason_out[g] = 1 road,
 * 2 flat count, 3 reversible-plies draw (0 if the game did not end); winner_out[g] = 0 white, 1 black, 2 draw.
 * Needed to write the PTN result of a Replay line (target.rs:215-232). */
int tz_search_terminal_details(tz_search* s, int8_t* reason_out, uint8_t* winner_out);
/* Validated move application without search (Replay::from_str / Replay::states, target.rs:205-212,248-268):
 * actions[g] (0xFFFF = none) is applied to game g iff it is legal there; ok_out[g] = 1 applied, 0 illegal or
 * none, -1 position already terminal.  Trees are reset.  Positions wider than max_actions are handled like any other up to 1024
 * legal moves, so on every board size but 6x6.  Of a 6x6 position with more, only the moves among the first 1024 or so (whole
 * squares' worth, in move order) are recognised: such a move is applied; for any other move, legal or not, ok_out[g] is 0, the
 * position is unchanged and the call returns TZ_ECAPACITY "more legal moves than max_actions" after handling the other games. */
int tz_search_play_moves(tz_search* s, const uint16_t* actions, int8_t* ok_out);
/* `steps` uniformly random legal moves for every game of the handle, from its current positions
 * (Environment::new_opening_with_random_steps after the opening, env.rs:81-95; eee/src/utils.rs reference_envs), in one launch.
 * The move of game g at a position is row[j] of its legal moves in move order, with
 *     u = mix64(mix64(mix64(seed) ^ (game_base + g)) ^ ply),   j = ((u >> 32) * n) >> 32,
 * mix64 = splitmix64's finaliser, ply = the position's own ply counter, n = the number of legal moves: integer arithmetic only,
 * and a playout made in two calls is the playout made in one.  A game stops before `steps` moves when it has no legal move
 * (env.rs:89-91), or, with TZ_RANDOM_STOP_AT_TERMINAL, when its position is terminal.  Without that flag the end of a game is not
 * looked at, as in the reference: random moves go on over a finished game for as long as there are any.
 * moves_out[g][i] / nlegal_out[g][i]: move i of game g and the number of legal moves it was drawn from; 0xFFFF / 0 from
 * played_out[g] on.  Any of the three may be NULL.  The trees of all games are reset (also of a game that played nothing); the
 * captured simulation graphs stay valid, as after tz_search_play_moves.
 * steps == 0 is valid and changes nothing.  TZ_EINVAL: steps < 0, unknown flag bits, a null handle.  A position with more than 1024
 * legal moves (6x6 only) ends its game's playout there, the position before that ply kept; the other games finish theirs and the
 * call returns TZ_ECAPACITY "more legal moves than max_actions".  A later call works again. */
#define TZ_RANDOM_STOP_AT_TERMINAL 1
int tz_search_random_steps(tz_search* s, uint64_t seed, uint64_t game_base, int steps, int flags,
                           uint16_t* moves_out /*[batch][steps] or NULL*/, uint16_t* nlegal_out /*[batch][steps] or NULL*/,
                           int32_t* played_out /*[batch] or NULL*/);
/* HashNetwork::forward_hash (net4_lcghash.rs:251-264) on the handle's current positions, without an upload: seen_out[g] = 1 if
 * the position's index is in the set (the reference's 0.0), 0 if not (MAXIMUM_VARIANCE).  The set is not updated.  TZ_EINVAL
 * unless the handle's agent is a loaded hash net (net4_simhash, net6_simhash, net4_lcghash). */
int tz_search_hash_seen(tz_search* s, uint8_t* seen_out /*[batch]*/);
/* BatchedMCTS::gumbel_sequential_halving with caller-supplied Gumbel(0,1) samples
 * (batched.rs:207-409): gumbel[batch][amax]; selected_out[batch] move indices. */
int tz_search_gumbel_sh(tz_search* s, const float* betas, int sampled_actions, int search_budget,
                        const float* gumbel, int amax, uint16_t* selected_out);
/* counters since creation: simulations (incl. Known hits) and network-evaluated leaves */
int tz_search_counters(tz_search* s, uint64_t* simulations, uint64_t* nn_leaf_evals);
/* The reference's trees are heap allocated and unbounded; a game's node pool here has `node_capacity` slots (default
 * 262 144 on 5x5: 66 GB for 4096 games).  When a leaf cannot get its children because the pool is full it is evaluated
 * and backed up without being expanded (it stays a leaf; the next tz_search_step compacts the kept subtree and frees
 * the rest), and the event is counted here.  With TZ_STRICT_CAPACITY set in the environment at creation a full pool is
 * TZ_ECAPACITY instead. */
int tz_search_pool_overflows(tz_search* s, uint64_t* skipped_expansions);
/* node slots in use in the fullest game's pool, and the per-game capacity */
int tz_search_pool_usage(tz_search* s, uint32_t* max_used, uint32_t* capacity);
int tz_search_sync(tz_search* s);
/* time spent (ms, HIP events on the handle's stream) in the dominant conv kernel and its
 * launch count since the last reset; used by bench.py for the roofline line. */
int tz_search_profile(tz_search* s, int reset, double* conv_ms, uint64_t* conv_launches,
                      double* tree_ms, uint64_t* steps);

/* ---------- selfplay::main above the search (selfplay/src/main.rs:63-387), native host code (csrc/tz_host.cpp) ----------
 * The outer loop of the reference's selfplay binary: search, move choice, take_a_step, restart_envs_and_complete_targets,
 * target / replay lines, buffer_lengths.txt back-pressure, append-only files.  Draws (openings, Dirichlet, Gumbel, early
 * move sampling) come from one seeded generator per (seed, shard).
 * search_kind: 0 PUCT + Dirichlet (:127-136), 1 Gumbel sequential halving (:138-153), 2 uniformly random moves
 * (learn's pre-training games, learn/src/main.rs:437-445).  exploration: cargo feature of that name (:79-86). */
typedef struct tz_selfplay tz_selfplay;
int tz_selfplay_create(tz_search* search, int sims_per_move, uint64_t seed, int shard, int search_kind, int sampled_actions,
                       int exploration, tz_selfplay** out);
int tz_selfplay_destroy(tz_selfplay* sp);
int tz_selfplay_play_move(tz_selfplay* sp);
int tz_selfplay_counters(tz_selfplay* sp, uint64_t* moves_out, uint64_t* targets_out, uint64_t* replays_out);
/* which: 0 target lines, 1 replay lines, 2 exploration replay lines finished since the last call */
int tz_selfplay_take_text(tz_selfplay* sp, int which, char* out, uint64_t cap, uint64_t* size_out);
/* the directory loop; reload(user) is called before every move (Net::load of model_latest, :107-121), may be NULL */
int tz_selfplay_run(tz_selfplay* sp, const char* directory, int moves, int max_buffer_len, const char* suffix,
                    int (*reload)(void*), void* reload_user, double wait_limit_s);

/* ---------- N shards: the exchange between the self-play processes of one job, csrc/tz_comm.cpp ----------
 * The reference runs N selfplay processes that append to the same files of one directory (README.md:130) and has no
 * collective.  With one process per GPU the shards hand over through a communicator: an all-gather of counts followed by
 * an all-gather of the packed target records / replay lines after every move, and a broadcast of a new model's weights.
 * Transports: RCCL (ncclAllGather / ncclBroadcast on the shard's GPU, xGMI inside a node; librccl is opened with dlopen on
 * first use) and "fs" (files in a shared directory, the reference's own medium: no GPU needed). */
typedef struct tz_comm tz_comm;
#define TZ_COMM_ID_BYTES 128
/* ncclGetUniqueId on one rank; the host carries the 128 bytes to the others (MPI, a TCP store, or the helper below) */
int tz_comm_unique_id(unsigned char* id_out /*[TZ_COMM_ID_BYTES]*/);
/* the same through `<directory>/rccl_id.bin`: rank 0 creates and publishes the id, the others wait for it */
int tz_comm_rendezvous_id(const char* directory, int rank, unsigned char* id_inout, double timeout_s);
/* ncclCommInitRank for this shard (collective over the world); device_id = the shard's GPU */
int tz_comm_create_rccl(const unsigned char* id, int rank, int world, int device_id, tz_comm** out);
int tz_comm_create_fs(const char* directory, int rank, int world, double timeout_s, tz_comm** out);
int tz_comm_destroy(tz_comm* c);
int tz_comm_info(tz_comm* c, int* rank_out, int* world_out, int* is_rccl_out, uint64_t* collectives_out, uint64_t* bytes_gathered_out);
/* variable-size all-gather of host bytes (counts, then padded payloads): sizes_out[world]; the payloads, back to back in
 * rank order (total_out bytes), stay with the handle until tz_comm_take copies them out */
int tz_comm_all_gather(tz_comm* c, const void* data, uint64_t bytes, uint64_t* sizes_out, uint64_t* total_out);
int tz_comm_take(tz_comm* c, void* out, uint64_t out_cap);
int tz_comm_broadcast(tz_comm* c, void* data, uint64_t bytes, int root);
int tz_comm_barrier(tz_comm* c);
/* Net::load for N shards (selfplay/src/main.rs:107-121): the root passes the result of its own load as `status` (0 = a new
 * model is active on it); every rank then takes the same branch: 0 = receive and activate those variables, else keep. */
int tz_net_broadcast(tz_net* net, tz_comm* c, int root, int status);
/* Self-play over N shards: with a communicator set, the targets a move finishes stay packed until tz_selfplay_exchange
 * (collective, once per tz_selfplay_play_move; tz_selfplay_run calls it) has gathered every rank's; afterwards rank
 * `writer_rank` (every rank if < 0) holds everybody's target / replay / exploration lines in rank order — for
 * tz_selfplay_take_text, or appended to the directory's files by tz_selfplay_run — and the other ranks hold none. */
int tz_selfplay_set_comm(tz_selfplay* sp, tz_comm* c, int writer_rank);
int tz_selfplay_exchange(tz_selfplay* sp);

/* ---------- reanalyze::main above the search (reanalyze/src/main.rs:60-290), native host code ----------
 * Position buffer fed from replays.txt (complete lines appended since the last call; line i belongs to rank i % world;
 * every pre-move state of a replay, moves re-validated on the device), B positions sampled without replacement,
 * fresh trees, search (0 = `sims` PUCT simulations, 1 = Gumbel sequential halving with budget `sims`), one target per
 * position: value = root evaluation if solved else -evaluation(selected child), policy =
 * improved_policy(most_visited_count()), ube = ube_target(0.25). */
typedef struct tz_reanalyze tz_reanalyze;
int tz_reanalyze_create(tz_search* search, int sims, uint64_t seed, int rank, int world, int search_kind, int sampled_actions,
                        tz_reanalyze** out);
int tz_reanalyze_destroy(tz_reanalyze* ra);
int tz_reanalyze_feed(tz_reanalyze* ra, const char* replays_path, uint64_t* added_out, uint64_t* total_out);
int tz_reanalyze_iterate(tz_reanalyze* ra);
int tz_reanalyze_take_text(tz_reanalyze* ra, char* out, uint64_t cap, uint64_t* size_out);
int tz_reanalyze_run(tz_reanalyze* ra, const char* directory, int iterations, int min_positions, const char* suffix,
                     int (*reload)(void*), void* reload_user, double wait_limit_s);

/* ---------- the other consumers of the search, native host code ----------
 * evaluation::compete (evaluation/src/main.rs:224-319): result_out[3] = wins, losses, draws for White. */
int tz_compete(tz_search* white, tz_search* black, const tz_state* games, float white_beta, float black_beta, uint64_t seed,
               int sampled_actions, int search_budget, int max_moves, int32_t* result_out);
/* puzzle benchmark (puzzle/src/main.rs:168-269): result_out[3] = attempted, solved, proven. */
int tz_puzzle_benchmark(tz_search* search, const tz_state* puzzles, const uint16_t* solutions, int count, int win, uint64_t seed,
                        int sampled_actions, int search_budget, int32_t* result_out);

/* ---------- Target lines in bulk (impl Display / FromStr for Target, target.rs:56-73, 99-143) ----------
 * "{tps};{value};{ube};{move}:{p},...\n" with Rust's `Display for f32`.  moves / policy are [count][amax]. */
int tz_format_targets(int n, int count, const tz_state* states, const uint16_t* moves, const float* policy,
                      const int32_t* nmoves, int amax, const float* value, const float* ube, char* out, uint64_t cap,
                      uint64_t* written_out);
/* parses the complete lines of text[0..len); unparsable lines are skipped (learn/src/main.rs:308);
 * consumed_out = bytes to advance the file offset by */
int tz_parse_targets(const char* text, uint64_t len, int n, int half_komi, int max_targets, int amax, tz_state* states,
                     uint16_t* moves, float* policy, int32_t* nmoves, float* value, float* ube, int32_t* count_out,
                     uint64_t* consumed_out, int32_t* skipped_out);

/* ---------- Trainer: the `learn` step (learn/src/main.rs:376-423), SURVEY.md 8f row 4 ----------
 * fp32 forward in training mode (BatchNorm batch statistics, running statistics updated with momentum 0.1),
 * masked log-softmax cross entropy + value MSE + UBE MSE, backward, Adam(lr) as tch's nn::Adam::default().
 * Tensors carry the VarStore names (`.a.` / `.b.` for the two SmallBlocks) and the reference's layouts.
 * batch must be a multiple of 64 (the reference uses 128, learn/src/main.rs:43). */
typedef struct tz_trainer tz_trainer;
int tz_trainer_create(int board_n, int arch, int device_id, int blocks, int batch, float learning_rate, tz_trainer** out);
int tz_trainer_destroy(tz_trainer* t);
int tz_trainer_tensor_count(tz_trainer* t);
int tz_trainer_tensor_info(tz_trainer* t, int i, char* name_out, int name_cap, uint64_t* count_out);
/* what: 0 parameter / buffer, 1 gradient of the last step, 2 / 3 Adam first / second moment */
int tz_trainer_set_tensor(tz_trainer* t, const char* name, int what, const float* data, uint64_t count);
int tz_trainer_get_tensor(tz_trainer* t, const char* name, int what, float* out, uint64_t count);
/* compute_loss_and_take_step: states[batch]; target_policy / mask [batch][tz_policy_size] (mask 1 = illegal,
 * move_mask); target_value[batch]; target_ube[batch] variances (ln + clamp to [-10, ln 4] applied inside,
 * learn/src/main.rs:360-363); train_ube = 0 in pre-training (:397-400); apply_step = 0 leaves the weights alone.
 * losses_out[3] = policy, value, ube. */
int tz_trainer_step(tz_trainer* t, const tz_state* states, const float* target_policy, const uint8_t* mask,
                    const float* target_value, const float* target_ube, int train_ube, int apply_step,
                    float* losses_out);
/* outputs of the last step's forward_t(xs, true): policy [batch][policy_size], value [batch], ube [batch] (log) */
int tz_trainer_outputs(tz_trainer* t, float* policy_out, float* value_out, float* ube_out);
/* what the last step's forward left after trunk layer `layer` (0 = input conv + BN + ReLU, then two per residual block, ReLU applied):
 * [batch][n*n][256] floats, pixel-major (NHWC).  out_cap in floats.  For tests: where an activation is zero the step's backward took
 * ReLU's derivative as zero — a comparison against another implementation can use the same side of the kink. */
int tz_trainer_activation(tz_trainer* t, int layer, float* out, uint64_t out_cap);

/* board size, batch and architecture of a trainer */
int tz_trainer_shape(tz_trainer* t, int* board_n_out, int* batch_out, int* arch_out);
/* Network::load / Network::save on the trainer's VarStore (learn/src/main.rs:107-120, 247-266): a LibTorch archive as tch
 * writes it or the .tzw container; variables the step never touches (RND nets, SimHash matrix) are carried through. */
int tz_trainer_load(tz_trainer* t, const char* path);
int tz_trainer_save(tz_trainer* t, const char* path);
/* tz_trainer_load from a .tzw container in memory (as tz_net_load_weights_mem) */
int tz_trainer_load_weights_mem(tz_trainer* t, const void* data, size_t bytes);
/* the carried variables (those the step never touches) as a .tzw container; bytes_out = its size, written to out only when
 * out is not NULL and cap holds it */
int tz_trainer_get_extras(tz_trainer* t, void* out, uint64_t cap, uint64_t* bytes_out);
/* the variables of a network (tz_net_init_random = Net::new, or a loaded model) become the trainer's, and back */
int tz_trainer_from_net(tz_trainer* t, tz_net* net);
int tz_trainer_to_net(tz_trainer* t, tz_net* net);

/* ---------- Training net4_ensemble's sixteen heads in the step (eee/src/ensemble.rs:318-351) ----------
 * targets[batch][16] (copied) arm the trainer: every later tz_trainer_step also runs the sixteen heads on the step's detached trunk
 * output in training mode, adds loss_ensemble = mean over [batch][16] of (target - value)^2, takes its gradient through the heads'
 * own variables only, and with apply_step runs Adam on them (a step count of their own).  NULL disarms.  While armed the 64
 * `ensemble head i.*` names answer to tz_trainer_get_tensor / _set_tensor (what 0..3).  With it never armed a trainer of this
 * architecture carries the heads through unchanged.  TZ_EINVAL unless TZ_ARCH_NET4_ENSEMBLE; TZ_ESTATE when the loaded variables
 * hold no `ensemble head i.*`.  The three losses and every gradient of the step itself are the same bytes armed or not: the heads
 * run after it, on its last activation. */
int tz_trainer_set_ensemble_targets(tz_trainer* t, const float* targets);
/* loss_ensemble and the heads' values [batch][16] of the last armed step (before its update); either may be NULL; TZ_ESTATE before one. */
int tz_trainer_ensemble_last(tz_trainer* t, float* loss_out, float* values_out);

/* ---------- Training net5's RND predictor in the step (net5.rs:193-218; learn/src/main.rs:404-405, 415-416) ----------
 * The reference ships loss_rnd = forward_rnd(input, true).mean() and update_rnd switched off by comments; here both are present
 * and off until asked for.  With it off a trainer does exactly what it did without these calls.
 * tz_trainer_rnd_enable: on != 0 switches the distillation step on.  tz_trainer_step then also runs both RND MLPs on x / sum(x^2)
 * of the batch's planes (net5.rs:126-127), takes loss_rnd = mean_b |learning - target|^2 (net5.rs:203, main.rs:404), its gradient
 * through the predictor only (the target is detached, net5.rs:197-202) and, with apply_step, Adam on the six rnd_learning.*
 * variables with a step count of their own (the feature may be switched on in the middle of a run; torch's Adam counts per
 * parameter).  train_ube has no bearing on it; rnd_target.*, min and max never change in a step.  While enabled, the six
 * rnd_learning.* names answer to tz_trainer_get_tensor / _set_tensor (what 0..3, weights as [out][in]); tz_trainer_tensor_count /
 * _info list what they always list.  Save, to_net and get_extras carry the current predictor; a load re-uploads the model's.
 * TZ_EINVAL unless the trainer is TZ_ARCH_NET5; TZ_ESTATE when the loaded variables hold no rnd_learning.* / rnd_target.* /
 * min / max. */
int tz_trainer_rnd_enable(tz_trainer* t, int on);
/* loss_rnd (main.rs:404) and forward_rnd (net5.rs:193-204) [batch] of the last step, computed before that step's update.
 * Either pointer may be NULL.  TZ_ESTATE before the first enabled step. */
int tz_trainer_rnd_last(tz_trainer* t, float* loss_out, float* raw_out /*[batch]*/);
/* What the last RND forward (a step's, or the last chunk of a calibration) left in an MLP (net5.rs:114-148): which 0 = learning,
 * 1 = target; layer 0, 1 = after the ReLU of input_linear / hidden_linear, [batch][1024]; 2 = the output, [batch][512].
 * out_cap in floats.  For tests, like tz_trainer_activation. */
int tz_trainer_rnd_activation(tz_trainer* t, int which, int layer, float* out, uint64_t out_cap);
/* update_rnd (learn/src/rnd_normalization.rs:74-78): min of forward_rnd over the early positions, max over the late ones (eval
 * mode, which for these MLPs is the training graph; any counts >= 1, processed in chunks of the trainer's batch).  apply != 0 stores
 * them in the variables min / max (update_rnd_normalization, net5.rs:213-218).  min_out / max_out may be NULL.
 * If !(max > min) the call returns TZ_ESTATE and, with apply set, leaves the variables alone.  The reference has no such guard:
 * it would store them, and normalized_rnd (net5.rs:206-211) would divide by zero.  TZ_ESTATE also while RND training is not
 * enabled. */
int tz_trainer_rnd_calibrate(tz_trainer* t, const tz_state* early, int n_early, const tz_state* late, int n_late, int apply,
                             float* min_out, float* max_out);

/* ---------- Training net4_rnd's predictor tower in the step (net4_rnd.rs:126-166, 210-223; residual.rs:8-63; learn/src/main.rs:404-405,
 * 415-416; eee/src/rnd.rs) ----------
 * Off until asked for: with it never enabled a trainer of this architecture carries the 106 tower variables unchanged and does, bit
 * for bit, what it did without these calls.
 * tz_trainer_rnd4_enable: on != 0 switches the distillation step on.  tz_trainer_step then also runs both towers on the batch's planes:
 * rnd_predictor in training mode (LayerNorm with the population variance, eps 1e-5; BatchNorm with the batch's mean and biased
 * variance over batch * 16 rows, eps 1e-5), rnd_target in eval mode (its running statistics), takes loss_rnd = mean_b sum_512
 * (predictor - target)^2 (net4_rnd.rs:210-223 with train = true, main.rs:404) and its gradient through the predictor only.  With
 * apply_step Adam (the trunk's lr, betas and eps) moves the predictor's 32 trained variables (LayerNorm weight and bias, then ten
 * times conv weight, BatchNorm weight, BatchNorm bias) with a step count of their own (the feature may be switched on in the middle
 * of a run), and the predictor's 20 running statistics move with momentum 0.1 and the unbiased variance (tch / torch).  With
 * apply_step = 0 the losses and gradients are computed and nothing else moves: no weight, no moment and, unlike the trunk's forward,
 * no running statistic of the tower.  train_ube has no bearing on it; rnd_target.*, min and max never change in a step.  Every sum
 * across workgroups is added in a fixed order: two runs give the same bits.
 * While enabled the predictor's 32 trained names answer to tz_trainer_get_tensor / _set_tensor (what 0..3, conv weights as
 * [co][ci][3][3]) and its 20 running statistics with what = 0; tz_trainer_tensor_count / _info list what they always list.  Save,
 * to_net, snapshot and get_extras carry the current predictor; a load re-uploads the model's towers.
 * TZ_EINVAL unless the trainer is TZ_ARCH_NET4_RND; TZ_ESTATE when the loaded variables hold no rnd_predictor.* / rnd_target.* /
 * min / max. */
int tz_trainer_rnd4_enable(tz_trainer* t, int on);
/* loss_rnd (main.rs:404) and forward_rnd(xs, true) (net4_rnd.rs:210-223) [batch] of the last enabled step, computed before that step's
 * update.  Either pointer may be NULL.  TZ_ESTATE before the first enabled step. */
int tz_trainer_rnd4_last(tz_trainer* t, float* loss_out, float* raw_out /*[batch]*/);
/* What the last enabled step left in a tower (net4_rnd.rs:126-166): which 0 = rnd_predictor, 1 = rnd_target.
 *   layer 0        the LayerNorm output, [batch][28][4][4]
 *   layer 1..10    the output of conv layer 1..10 (input conv, res_block_0.a, res_block_0.b, .., res_block_3.b, last_small_block) after
 *                  BatchNorm, the residual add and ReLU (none after layer 10), [batch][16 squares][32 channels]
 *   layer 11..20   predictor only: the conv output of layer 1..10 before BatchNorm, [batch][16][32]
 * out_cap in floats.  For tests, like tz_trainer_activation. */
int tz_trainer_rnd4_activation(tz_trainer* t, int which /*0 predictor, 1 target*/, int layer, float* out, uint64_t out_cap);
/* update_rnd (learn/src/rnd_normalization.rs:74-78): min of forward_rnd(xs, false) over the early positions, max over the late ones,
 * both towers in eval mode (the predictor with its current running statistics); any counts >= 1, in chunks of the trainer's batch.
 * Computed by the inference library's own TZ_PREC_F32 tower on the trainer's current variables folded as a model's are, so the
 * values are exactly what the saved model returns from tz_net_rnd_raw in that precision.  apply != 0 stores them in the variables
 * min / max (update_rnd_normalization, net4_rnd.rs:232-237).  min_out / max_out may be NULL.  If !(max > min) the call returns
 * TZ_ESTATE and, with apply set, leaves the variables alone (as tz_trainer_rnd_calibrate).  TZ_ESTATE also while not enabled. */
int tz_trainer_rnd4_calibrate(tz_trainer* t, const tz_state* early, int n_early, const tz_state* late, int n_late, int apply,
                              float* min_out, float* max_out);

/* ---------- learn::main above the step (learn/src/main.rs:99-319, 486-516), native host code (csrc/tz_host_learn.cpp) ----------
 * The two target buffers with forced-use counts (SELFPLAY / REANALYZE_TARGET_FORCED_USES, :59-60) fed by tailing the
 * target files, create_batch (uniform sampling without replacement, a random board symmetry per target, dense
 * policy / mask tensors) and the training loop with buffer_lengths.txt.  which: 0 selfplay, 1 reanalyze. */
typedef struct tz_learn tz_learn;
int tz_learn_create(tz_trainer* trainer, int half_komi, uint64_t seed, int selfplay_forced_uses, int reanalyze_forced_uses,
                    tz_learn** out);
int tz_learn_destroy(tz_learn* l);
int tz_learn_feed(tz_learn* l, int which, const char* path, int model_steps, uint64_t* added_out);
int tz_learn_add_lines(tz_learn* l, int which, const char* text, uint64_t len, int model_steps, uint64_t* added_out);
int tz_learn_buffer_len(tz_learn* l, int which, uint64_t* len_out);
int tz_learn_step(tz_learn* l, int using_reanalyze, int train_ube, int augment, float* losses_out);
/* Diagnostic: the tensors of the batch tz_learn_step built last (any pointer may be NULL) */
int tz_learn_last_batch(tz_learn* l, tz_state* states_out, float* policy_out, uint8_t* mask_out, float* value_out, float* ube_out);
/* the main loop (:172-269); on_step(user, model_steps, losses[3], batch states, batch) runs after every step (save
 * points and SimHash update_counts live there); a non-zero return stops the loop */
int tz_learn_run(tz_learn* l, const char* directory, int64_t starting_steps, int64_t steps, int min_selfplay, int min_reanalyze,
                 int64_t steps_before_reanalyze, double read_interval_s, double sleep_s, double wait_limit_s,
                 int (*on_step)(void*, int64_t, const float*, const tz_state*, int), void* user, int64_t* model_steps_out);
/* The save points of learn::main inside tz_learn_run (learn/src/main.rs:247-266): `model_latest.ot` every steps_per_save
 * steps (100 in the reference), `model_<steps>.ot` every steps_per_checkpoint (50 000), as LibTorch archives written behind
 * the training loop; hash_net (may be NULL): a SimHash net whose set is updated with every batch (:418) and saved as
 * `bitvec.bin` beside the model.  0 = no such save point. */
int tz_learn_set_save_points(tz_learn* l, int steps_per_save, int steps_per_checkpoint, tz_net* hash_net);
/* RND training inside the loop (learn/src/main.rs:404-405, 415-416): train_rnd != 0 enables it on the loop's trainer
 * (tz_trainer_rnd_enable, or tz_trainer_rnd4_enable / _calibrate when the trainer is TZ_ARCH_NET4_RND; 0 disables it), so every step
 * of tz_learn_step / tz_learn_run trains the predictor.  early / late (copied;
 * may be NULL with a count of 0) are the reference positions of update_rnd: with them, tz_learn_run calibrates with apply = 1
 * immediately before every model file it writes and before every on_step callback that falls on a multiple of calibrate_every
 * (> 0), so that a saved model's min / max belong to its weights.  The commented-out reference calibrates after every step: two
 * extra forwards of 256 positions for values that only a saved model hands on. */
int tz_learn_set_rnd(tz_learn* l, int train_rnd, const tz_state* early, int n_early, const tz_state* late, int n_late,
                     int calibrate_every);
/* reference_games (learn/src/rnd_normalization.rs:23-58): game i of n_early plays early_ply + i % 2 uniformly random legal moves
 * from the empty board, game i of n_late late_ply + i % 2 (the reference: 256 at ply 4, 256 at ply 120); the positions reached go
 * to early_out[n_early] / late_out[n_late].  Played on `search` (any agent kind; its positions and trees are overwritten) with the
 * calls of pre-training's random games.  Draws come from a counter-based generator keyed by (seed, game, ply): the reference's
 * stream is unpinned.  A game that ends early contributes its last non-terminal position (the net never sees a terminal one; the
 * reference keeps the terminal position, which is unpinned too). */
int tz_learn_rnd_reference(tz_search* search, uint64_t seed, int n_early, int early_ply, int n_late, int late_ply,
                           tz_state* early_out, tz_state* late_out);

/* ---------- tei: the reference's engine binary (tei/src/main.rs, tei/src/protocol.rs), native host code (csrc/tz_tei.cpp) ----------
 * A UCI-style text engine over ONE tree: the session keeps a game, replays `position` commands with tree reuse
 * (tz_search_step_wide), and searches with tz_search_simulate_batch(leaves, rounds = 1) at beta 0 until a node count, a move time
 * or a stop ends it (main.rs:139-297).  examples/tei_cli.cpp is the program around it (handshake, reader thread).
 *
 * tz_tei_create: one_tree must have a batch of 1 (else TZ_EINVAL) and a net or dummy agent; leaves is BATCH_SIZE of main.rs:26
 * (128).  Like the reference (main.rs:141) it runs one simulation on the start position.  The session borrows the handle; destroy
 * the session first.
 *
 * tz_tei_line: one input line after the handshake (isready, teinewgame N, position startpos|tps ... [moves ...], go ..., stop,
 * quit; tei and setoption get a warning).  The output lines, each ended by '\n', are written to out[cap] with a final NUL;
 * *size_out = their length (if it exceeds cap - 1, out holds the first cap - 1 bytes).  *quit_out = 1 when the program should end.
 * `go` returns when the search has ended, with its info line or lines and `bestmove`.  What the reference writes to its log
 * (stderr) comes out as `info string error: ...` / `info string warning: ...` lines.  An unparsable line is TZ_EPARSE with such a
 * line; the session is unchanged.
 *
 * `position`: when the position equals the last one and the move list starts with the last move list, the tree is kept
 * (main.rs:174-184): every new move must be among the root's children and is applied with tz_search_step_wide; on a root without
 * children it goes through tz_search_play_moves, which validates it and resets the tree (Node::descend on a childless node).
 * Otherwise the tree is reset, the position set and the moves played with tz_search_play_moves.  A move that is not legal stops
 * the replay with an error line.
 *
 * `go`: nodes N, movetime ms, infinite, and wtime / btime / winc / binc taken for the side to move only (:216-236); with both the
 * mover's time and increment and no movetime, movetime = time / 10 + 3 * inc / 4 (:241-243).  After every round: visits = root
 * visits - visits at the start; done when visits >= nodes or elapsed >= movetime; an info line when the info interval has passed
 * (:251-279).  At the end an info line if none was sent, then `bestmove` (tz_search_select_best_actions); the limits are cleared.
 *
 * Where the session leaves the reference:
 *   - nps is 0 when the time is 0 ms (the reference divides by zero);
 *   - teinewgame also forgets the last position and move list (the reference keeps them, and a new game whose moves extend the
 *     old list would be replayed from the wrong position); so does a `position` whose replay met an illegal move;
 *   - `go` on a root without children (a terminal position; an over-wide one is TZ_ECAPACITY from the search call) gives no
 *     bestmove: an `info string` line and TZ_ESTATE;
 *   - before every round, if capacity - max_used < leaves * max_actions (tz_search_pool_usage, tz_search_shape; the most one
 *     round can allocate) the search ends as `stop` would, with `info string node pool full`: the reference's heap has no bound,
 *     and expansions skipped silently (tz_search_pool_overflows) would make a long think worthless;
 *   - a `stop` line outside a search prints nothing (the reference prints an info line and a bestmove).
 *
 * tz_tei_stop is the only call allowed from a second thread while tz_tei_line runs.  It announces a `stop` or `quit` line that the
 * caller passes to tz_tei_line in its turn: a search ends after the round in progress while a stop has been announced whose line
 * has not been passed yet.  (So `go`, `stop`, `go`, `stop` read faster than they are handled end both searches, and a `stop` that
 * arrives between two searches does not cut the second one short.)
 *
 * tz_tei_set_sink: with a sink, the info lines of a search go to sink(user, line) as they arise (line without '\n') instead of
 * to `out`; a non-zero return ends the search as `stop` would.  tz_tei_set_info_interval: milliseconds between info lines,
 * default 300 (main.rs:24). */
typedef struct tz_tei tz_tei;
int tz_tei_create(tz_search* one_tree, int leaves, tz_tei** out);
int tz_tei_destroy(tz_tei* t);
int tz_tei_line(tz_tei* t, const char* line, char* out, uint64_t cap, uint64_t* size_out, int* quit_out);
int tz_tei_stop(tz_tei* t);
int tz_tei_set_sink(tz_tei* t, int (*sink)(void*, const char*), void* user);
int tz_tei_set_info_interval(tz_tei* t, int ms);
/* Input::from_str (protocol.rs:74-160) for board size n, without a device.  *kind_out = TZ_TEI_*; numbers_out[8]:
 *   teinewgame: [0] = size;  position: [0] = 0 startpos, 1 tps (tps_out = the three TPS words joined by spaces), moves_out /
 *   *n_moves_out = the move indices (TZ_EINVAL if more than moves_cap);  setoption: tps_out = "<name> <value>";
 *   go: [0] = mask of the options given, bit TZ_TEI_GO_*; [1 + TZ_TEI_GO_*] = the option's number (ms, or nodes).
 * A line that does not parse returns TZ_EPARSE with *kind_out = TZ_TEI_ERROR, numbers_out[0] = TZ_TEI_ERR_* (ParseInputError) and
 * its text in tz_last_error. */
#define TZ_TEI_ERROR (-1)
#define TZ_TEI_TEI 0
#define TZ_TEI_ISREADY 1
#define TZ_TEI_SETOPTION 2
#define TZ_TEI_NEWGAME 3
#define TZ_TEI_POSITION 4
#define TZ_TEI_GO 5
#define TZ_TEI_STOP 6
#define TZ_TEI_QUIT 7
#define TZ_TEI_GO_WTIME 0
#define TZ_TEI_GO_BTIME 1
#define TZ_TEI_GO_WINC 2
#define TZ_TEI_GO_BINC 3
#define TZ_TEI_GO_MOVETIME 4
#define TZ_TEI_GO_NODES 5
#define TZ_TEI_GO_INFINITE 6
#define TZ_TEI_ERR_MISSING_FIRST_WORD 1
#define TZ_TEI_ERR_MISSING_NAME 2
#define TZ_TEI_ERR_MISSING_VALUE 3
#define TZ_TEI_ERR_MISSING_SIZE 4
#define TZ_TEI_ERR_PARSE_INT 5  /* ParseSize: every number of the protocol (ParseIntError) */
#define TZ_TEI_ERR_MISSING_POSITION 6
#define TZ_TEI_ERR_MISSING_TPS 7
#define TZ_TEI_ERR_PARSE_TPS 8
#define TZ_TEI_ERR_PARSE_MOVE 9
#define TZ_TEI_ERR_MISSING_SECONDS 10
#define TZ_TEI_ERR_MISSING_AMOUNT 11
#define TZ_TEI_ERR_UNRECOGNIZED 12
int tz_tei_parse(const char* line, int n, int* kind_out, int64_t* numbers_out, uint16_t* moves_out, int moves_cap, int* n_moves_out,
                 char* tps_out, int tps_cap);
/* Output::Info's Display (protocol.rs:240-274): "info time <ms> nodes <n> nps <1000 * n / ms> wdl <w> <d> <l>[ score mate <+-m>]
 * score cp <c> pv <moves in PTN>": wdl 1000 0 0 / 0 0 1000 / 0 1000 0 for Win / Loss / Draw and 500 + round(v * 500), 0, the rest
 * for a value v; score mate +-ceil(ply / 2) for a proven win or loss only; cp = round(f32::from(eval) * 100), halves away from
 * zero, f32::from(Eval) being the value or +-0.997^ply (0 for a draw).  Without a device.  Returns the length written (without the
 * NUL), TZ_EINVAL if cap is too small. */
int tz_tei_format_info(int n, uint64_t time_ms, uint64_t nodes, uint8_t eval_tag, uint32_t eval_bits, const uint16_t* pv, int pv_len,
                       char* out, int cap);

/* Diagnostic: evaluates on the device the f32 primitives the tree kernels must compute exactly as
 * the host does (op 0 exp, 1 ln, 2 sqrt, 3 a/b, 4 0.997^int(a), 5 (a+b)*a). */
int tz_device_math(int op, const float* a, const float* b, float* out, int n);
/* Diagnostic: average ms per launch of the 5x5 residual-tower conv kernel on `positions` boards;
 * variant 0 = the shipped kernel, 1/2/3 = ablations (no LDS reads / no weight loads / neither). */
int tz_debug_conv_bench(tz_net* net, int variant, int positions, int iters, float* ms_out);
/* Diagnostic: the same for the fused residual-tower kernel (variant = its OPT bitmask). */
int tz_debug_tower_bench(tz_net* net, int variant, int positions, int iters, float* ms_out);
/* Diagnostic: average ms per launch of a hash net's index-plus-lookup kernel (simhash_state_kernel / lcghash_state_kernel) on
 * `batch` positions, between two events around `iters` launches after two warm-up launches. */
int tz_debug_hash_bench(tz_net* net, int batch, const tz_state* states, int iters, float* ms_out);
/* the same for the tower kernel of TZ_ARCH_NET4_RND (both towers and the variance rule): milliseconds per launch over `batch` positions */
int tz_debug_rnd4_bench(tz_net* net, int batch, const tz_state* states, int iters, float* ms_out);
/* Diagnostic (builds with --ablations, TZ_NET_ABL=8): in-kernel shader clock of the last stamped launch of the net kernel
 * (median over workgroups of delta s_memtime / delta s_memrealtime x 100 MHz) and the median duration of its tower part. */
int tz_debug_net_clock(tz_net* net, double* mhz_out, double* tower_us_out);
/* diagnostic builds: the raw in-kernel stamps of the last stamped launch, [workgroup][4] (TZ_NET_ABL=8: memtime, memrealtime before
   and after the tower; TZ_NET_ABL=16: memtime after the barrier, the k-loop, the barrier and the epilogue of the middle layer) */
int tz_debug_net_stamps(tz_net* net, unsigned long long* out, int max_groups, int* groups_out);

#ifdef __cplusplus
}
#endif
#endif /* TAKZERO_HIP_H */
