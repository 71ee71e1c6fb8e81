/*
 * hive_search.h -- C ABI of the GPU-resident tree search (libhive_hip.so).
 *
 * Replaces the reference's per-process MCTS for the throughput path:
 *   woker/solo_play.py::HivePlayer (:69-384)   search_my_move / select_action_q_and_u / calc_policy
 *   woker/self_play.py::self_play_buffer (:116-193)   move selection rules of the self-play loop
 * One tree per game lives in a flat SoA node pool in HBM; G games are searched in lock step, one
 * leaf per game (and per in-flight slot) per simulation, so the network sees batches of G leaves
 * (woker/api_hive.py:47-74 batched whatever arrived within 1 ms).
 *
 * Division of labour per simulation:
 *   hive_search_select   PUCT descent + virtual loss (solo_play.py:199-208,294-335); writes the leaf
 *                        positions (parent record + apply_action) into caller buffers
 *   -- caller: hive_encode_launch / hive_movegen_launch / terminal on the leaves, then the network --
 *   hive_search_backup   expansion (priors masked + renormalised, solo_play.py:304-313) and the
 *                        value backup with the reference's draw sentinel (solo_play.py:217-247)
 *
 * Differences from the reference, by design: an explicit node pool per game instead of a
 * dict keyed by state_key (transpositions are merged through a hash table, see below); fp32 statistics; the
 * Dirichlet noise comes from a counter-based generator, not numpy's stream.  The reference-exact sequential
 * search is hive-alphazero_amd/solo_play.py.
 *
 * All pointers are DEVICE pointers; the caller allocates leaf/policy buffers, the handle owns the
 * node pool.  Return codes and hive_last_error() as in hive_abi.h.
 */
#ifndef HIVE_SEARCH_H
#define HIVE_SEARCH_H

#include <stdint.h>

#include "hive_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIVE_EDGE_CAP 256      /* edges stored per node (legal ids beyond it are dropped; max seen: 131) */
#define HIVE_MAX_SLOTS 8       /* in-flight leaves per tree */

typedef struct HiveSearch HiveSearch;

/* Which of the reference's two searches the kernels run. */
typedef enum {
    HIVE_SEARCH_PUCT = 0,  /* woker/solo_play.py::HivePlayer (:167-374): q = w/n, u = c_puct p sqrt(sum_n + 1)/(1 + n), priors masked
                              and renormalised, root Dirichlet noise per simulation, draw sentinel, length cap, state_key merging */
    HIVE_SEARCH_UCT = 1    /* alpha_zero/MCTS_chess.py::UCTNode/UCT_search (:52-151): Q = W/(1 + N), U = sqrt(N_node) |P|/(1 + N)
                              (c = 1), illegal priors zeroed WITHOUT renormalisation, no noise, plain tree, the backup adds
                              +v to edges played by white and -v to edges played by black (:111-119), a finished game or a
                              position without legal moves is re-evaluated by the network on every visit (:144-146, :87-88),
                              no length cap.  All score arithmetic in fp32 with the reference's operation order. */
} HiveSearchMode;

typedef struct HiveSearchParams {
    float c_puct;          /* solo_play.py:26   0.7  */
    float noise_eps;       /* solo_play.py:29   0.25 */
    float dirichlet_alpha; /* solo_play.py:28   0.3  */
    int32_t max_game_length; /* hive_engine/config.py:22  55 */
    int32_t mode;          /* HiveSearchMode */
    float virtual_loss;    /* solo_play.py:30   1 (n += 1, w -= virtual_loss while a simulation is in flight).  UCT with one
                              slot: 0, which keeps W bit-identical to the reference's sequential sums */
} HiveSearchParams;

int hive_search_create(int games, int max_nodes, int slots, int device, uint64_t seed, HiveSearch **out);
int hive_search_destroy(HiveSearch *s);
int hive_search_set_stream(HiveSearch *s, void *stream);
int hive_search_set_params(HiveSearch *s, const HiveSearchParams *p);

/* Start a new search from these positions (HivePlayer.action -> reset, solo_play.py:110-116).
 * active = int8[games] or NULL: games with active == 0 are skipped by every later call. */
int hive_search_set_roots(HiveSearch *s, const HiveBoard *boards, const HiveHistory *hist, const int8_t *active);

/* Start the next search from the subtree under the move that was played, instead of from nothing (the reference empties
 * its tree on every move, solo_play.py:103-112; this is opt-in).  played = int32[games] or NULL: the action id (-1 = pass)
 * that led from the root of game g's previous search to boards[g]; -3 (and NULL) = an unrelated position.  boards / hist /
 * active as hive_search_set_roots.
 * Game g keeps its tree iff it is active, its old root has an edge with that action whose child c exists (>= 0), c is not
 * a finished game, the position key of c (bytes 0..32 + turn parity, see hive_search_set_transpositions) equals that of
 * boards[g], and kept + sims_room <= max_nodes (hive_search_set_carry_room).  Every other game is left exactly as
 * hive_search_set_roots leaves it.
 * A kept tree holds the nodes reachable from c through expanded edges (child >= 0), c as node 0, renumbered breadth first
 * in edge order; every node keeps its records, nedge, sum_n, term, tv and its edges' act / p / n / w bit for bit, child is
 * renumbered.  The one exception: node 0's HiveBoard / HiveHistory become boards[g] / hist[g] -- the key holds neither the
 * turn number nor the history, and the simulations start from node 0's records.  The transposition table is rebuilt over the
 * kept nodes.  Out of place: the kept nodes move into a second node pool (allocated by the first call, same size as the
 * first) and the handle swaps the two.  Any search mode; max_nodes <= 8192. */
int hive_search_advance_roots(HiveSearch *s, const int32_t *played, const HiveBoard *boards, const HiveHistory *hist,
                              const int8_t *active);

/* Nodes a kept tree must leave free for the next search (default: slots + 2; a caller that runs `sims` simulations per
 * search passes sims + slots + 2).  A tree that would leave less is dropped and counted in `refused`. */
int hive_search_set_carry_room(HiveSearch *s, int sims_room);

/* int32[games] each (any may be NULL): kept_nodes = nodes kept by the last hive_search_advance_roots (0 = fresh tree),
 * carried_visits = sum_n of the new root carried over by it, refused = trees dropped for lack of room since create. */
int hive_search_carry_stats(HiveSearch *s, int32_t *kept_nodes, int32_t *carried_visits, int32_t *refused);

/* One game's tree for tests and tools, copied into caller-owned device buffers (any may be NULL): n_nodes = int32[1];
 * boards / hist / nedge / sum_n / term / tv = [max_nodes]; e_act / e_p / e_n / e_w / e_child = [max_nodes][HIVE_EDGE_CAP].
 * Only the first n_nodes rows, and of a row's edges the first nedge, are meaningful.  e_child: node index, -1 = not
 * expanded, -2 = expansion in flight (only between hive_search_select and hive_search_backup). */
int hive_search_export_tree(HiveSearch *s, int game, int32_t *n_nodes, HiveBoard *boards, HiveHistory *hist, int32_t *nedge,
                            int32_t *sum_n, int8_t *term, float *tv, int16_t *e_act, float *e_p, int32_t *e_n, float *e_w,
                            int32_t *e_child);

/* The value every node of one game's tree was created with, for tests and tools: node_v = float[max_nodes], of which only
 * the first n_nodes entries (hive_search_export_tree) are meaningful.  A node that is not a finished game holds the network's
 * value of its own position from the side to move there (the v of the hive_search_backup that created it; node 0: the
 * root's); a finished game or a position at the length cap holds its tv.  Written for every node in every mode;
 * hive_search_advance_roots moves it with the kept nodes like tv. */
int hive_search_node_values(HiveSearch *s, int game, float *node_v);

/* Selection for in-flight slot `slot`: leaf_boards / leaf_hist = [games] records of the positions to
 * evaluate (untouched for games whose path ended in a known terminal node or a collision). */
int hive_search_select(HiveSearch *s, int slot, HiveBoard *leaf_boards, HiveHistory *leaf_hist);

/* Expansion + backup for slot `slot`.  leaf_mask = uint32[games][HIVE_MASK_WORDS] legal sets of the leaves (destination boards, hive_abi.h),
 * over / winner as hive_batch_terminal, p = float[games][1584] (softmax output), v = float[games]. */
int hive_search_backup(HiveSearch *s, int slot, const HiveBoard *leaf_boards, const HiveHistory *leaf_hist,
                       const uint32_t *leaf_mask, const int8_t *over, const int8_t *winner, const float *p,
                       const float *v);

/* Which leaves of the last hive_search_select calls (slots 0 .. slots-1, after hive_leaf_launch filled `over`) will
 * hive_search_backup ask the evaluator about?  need = int8[slots * games] (1 = the network's p / v of that row are read;
 * 0 = finished game, length cap, revisited terminal node, collision or idle tree: solo_play.py:169-183 take those values
 * without a prediction, and the reference never calls its model for them -- api_hive.py:62-69 is reached only from
 * solo_play.py:188-197).  leaf_boards / over are the full [slots * games] arrays.  total (may be NULL): uint64 device
 * counter, the number of rows flagged 1 is ADDED to it.  Feed `need` to hive_nn_conv3x3_sel / hive_nn_resblock_sel. */
int hive_search_leaf_need(HiveSearch *s, int slots, const HiveBoard *leaf_boards, const int8_t *over, int8_t *need,
                          uint64_t *total);

/* HivePlayer.calc_policy + apply_temperature (solo_play.py:337-374) at the roots:
 * policy = float[games][1584] visit distribution (may be NULL), action = int32[games] (argmax, -1 = pass),
 * sum_n = int32[games] (may be NULL).  selfplay != 0 adds self_play.py:139-157: for turn <= 6 the
 * move is resampled from (1 - e) * policy + e * Dirichlet(0.5) over the legal moves, e = 0.7 - 0.15 * int(turn+1)/2. */
int hive_search_policy(HiveSearch *s, float *policy, int32_t *action, int32_t *sum_n, int selfplay);

/* The reference's tree is a dict keyed by GamePlay.state_key (solo_play.py:167-197; the key holds the pieces of every
 * cell bottom->top and the side to move, not the turn number or the history): a position reached by two move orders is
 * ONE entry with shared statistics.  merge != 0 (the default) gives the GPU tree the same semantics through a per-game
 * hash table over bytes 0..32 + turn parity of the HiveBoard record; merge == 0 keeps a plain tree.
 * hive_search_transposition_hits: int32[games], descents that continued through such a shared node since create. */
int hive_search_set_transpositions(HiveSearch *s, int merge);
int hive_search_transposition_hits(HiveSearch *s, int32_t *hits);

/* Statistics for tests: nodes allocated per tree (int32[games]). */
int hive_search_node_counts(HiveSearch *s, int32_t *counts);

/* Global game index of every tree (device int64[games]; default: 0 .. games-1).  The Dirichlet / resampling streams of
 * game i are keyed on (seed, ids[i], turn of the root position, simulation number inside the search, slot, edge) and on
 * nothing else, so a self-play game comes out the same whichever batch slot, process or GPU runs it
 * (seed = base + global_game_index; woker/self_play.py:37-75 seeds nothing and is not reproducible). */
int hive_search_set_game_ids(HiveSearch *s, const int64_t *ids);

/* Root statistics as the reference's UCTNode arrays (alpha_zero/MCTS_chess.py:33-35): visits / total_value / priors =
 * float[games][1584] each (any may be NULL), zero outside the root's edges.  PUCT mode: n, w, p of the root entry
 * (solo_play.py:51-66). */
int hive_search_root_stats(HiveSearch *s, float *visits, float *total_value, float *priors);

/* Leaves by kind since create: int32[games][8], every simulation of an active game adds one: [1] root evaluated,
 * [2] new position evaluated (1 + 2 = the network evaluations the search NEEDED), [3] descent ended in a known finished
 * game, [4] collision between in-flight slots, [5] descent ended at the length cap, [6] new position that is a finished
 * game or sits at the length cap (PUCT: its value does not come from the network), [7] new position that another
 * in-flight slot had already created.  [0] unused. */
int hive_search_leaf_histogram(HiveSearch *s, int32_t *hist);

/* Per-game simulation budgets.  budget = DEVICE int32[games], quiet = DEVICE int8[games] (or NULL); the caller owns both and
 * the handle keeps the pointers until the next call.  NULL, NULL (the default) switches the feature off.
 * budget[g] = the simulations game g gets in each search: hive_search_select number `sim` of a search (0, 1, 2, ...: the
 * count since hive_search_set_roots / hive_search_advance_roots, over all slots) treats a game with sim >= budget[g] exactly
 * as an inactive one -- no leaf, no virtual loss, no histogram entry; hive_search_backup and hive_search_leaf_need then skip
 * its row.  quiet[g] != 0 switches the root Dirichlet noise off for game g alone; the noise key of every other game is
 * untouched.  Either search mode, any slots, with and without hive_search_advance_roots.
 * The invariant: with the rounds of simulations laid out as TreeSearch lays them out (simulation 0 alone, then `slots` per
 * round), a game with budget b <= sims ends a search of `sims` simulations with the tree a search of b simulations of the
 * same batch gives it, bit for bit -- the noise is keyed on the simulation number, not on the batch.
 * budget <= 0: the game gets no simulation; a fresh root then has no tree and hive_search_policy answers -2 for it (a tree
 * kept by hive_search_advance_roots answers from the visits it carried). */
int hive_search_set_budgets(HiveSearch *s, const int32_t *budget, const int8_t *quiet);

/* Playout-cap randomisation: is this ply of game g searched in full or fast?  One thread per game; x = the first output of
 * the search's counter-based generator keyed (seed ^ 0x8CB92BA72F3D8DD7, game_id[g], root turn, 0); the ply is full iff
 * (x >> 32) < full_threshold, and always when full_threshold = 0xFFFFFFFF -- the host passes floor(p_full * 2^32), saturated.
 * A pure function of (seed, game id, turn): not of the slot, batch size, process or GPU.  game_id = int64[n], root_boards =
 * HiveBoard[n], active = int8[n] or NULL.  budget[g] (int32[n]) = full_sims or fast_sims, full[g] (int8[n], may be NULL) =
 * 1 or 0, quiet[g] (int8[n], may be NULL: the caller does not want quiet fast plies) = !full[g]; a game with active == 0
 * gets 0 in all three. */
int hive_search_draw_budgets(uint64_t seed, const int64_t *game_id, const HiveBoard *root_boards, const int8_t *active, int n,
                             int full_sims, int fast_sims, uint32_t full_threshold, int32_t *budget, int8_t *quiet, int8_t *full,
                             void *stream);

/* ---- Rolling search: every game on its own clock.
 *
 * on != 0 gives the handle a device int32 clock[games] (zeroed by this call): clock[g] = the simulations game g's current
 * search has run, in place of the one host counter that numbers the simulations of a lock-step batch.  A round is then
 *   hive_search_select(slot 0 .. slots-1) -> leaves, network -> hive_search_backup(slot 0 .. slots-1) -> hive_search_round_end
 * and with c = clock[g], b = budget[g] (hive_search_set_budgets: required, hive_search_select returns HIVE_E_ARG without)
 * game g takes part in slot sl iff it is active, c + sl < b and (c > 0 or sl == 0) -- the root-opening simulation runs
 * alone, as in a lock-step search.  Otherwise the slot treats it exactly as an inactive game: no leaf, path length 0, no
 * virtual loss, no histogram entry.  Its simulation number for the noise key is c + sl: 0 alone, then 1 + sl,
 * 1 + slots + sl, ... -- the numbers a lock-step search gives the same simulations, so game g ends its search with the tree
 * a lock-step search of budget[g] simulations gives it, bit for bit, whatever its neighbours do meanwhile.
 * The caller changes budget[g] / quiet[g] only between a `done` for game g and its restart.
 * hive_search_set_roots restarts every game (clocks 0); hive_search_advance_roots returns HIVE_E_ARG while on: it moves all
 * trees at once.  on == 0 goes back to the host counter. */
int hive_search_set_rolling(HiveSearch *s, int on);

/* After the backups of a round of `slots_run` slots: an active game with clock < budget advances by 1 if its clock was 0,
 * else by min(slots_run, budget - clock).  done = int8[games]: 1 for an active game whose clock has reached its budget (it
 * stays 1, and the game sits out, until hive_search_restart), 0 for every other game. */
int hive_search_round_end(HiveSearch *s, int slots_run, int8_t *done);

/* hive_search_set_roots for the games with which[g] != 0 (int8[games]) alone: root, empty tree and table, active flag,
 * clock 0; boards / hist / active are read at those games only.  Every other game keeps every byte of its state. */
int hive_search_restart(HiveSearch *s, const int8_t *which, const HiveBoard *boards, const HiveHistory *hist,
                        const int8_t *active);

/* hive_search_policy for the games with which[g] != 0 (int8[games]); every other game is answered as an inactive one:
 * zero policy row, action -2, sum_n 0.  With or without hive_search_set_rolling. */
int hive_search_policy_where(HiveSearch *s, const int8_t *which, float *policy, int32_t *action, int32_t *sum_n, int selfplay);

/* The clocks, copied into device int32[games]. */
int hive_search_clocks(HiveSearch *s, int32_t *clock);

/* ---- Gumbel root with sequential halving ("Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022; the
 * schedule follows the published mctx implementation).  Opt-in, PUCT mode, ROOT ONLY: below the root the descent is the PUCT
 * of hive_search_select without noise (the paper's root-only variant; non-root Gumbel selection is not built).
 * hive_search_set_gumbel_interior, further down, lifts that restriction for the games it names: it is a call of its own and
 * this block describes the search without it.
 *
 * The rule.  A root has edges e = 0 .. ne-1 in ascending action id with visits N_e, value sums W_e and priors P_e
 * (renormalised over the legal moves); v_root is the network's value of the root position.
 *   logit_e = logf(max(P_e, 1e-30f))
 *   g_e     = 0 for a quiet game (hive_search_set_budgets), else -logf(-logf(u_e)), u_e = the first uniform of the search's
 *             counter-based generator keyed (seed ^ 0x6A09E667F3BCC909, game id, root turn, simulation 0, slot 0, edge e):
 *             one draw per edge and search, a pure function of its keys like every other draw here
 *   q_e     = W_e / N_e where N_e > 0;  SN = sum of N_e
 *   v_mix   = v_root if SN == 0, else (v_root + SN * (sum over N_b > 0 of P_b q_b) / (sum over N_b > 0 of P_b)) / (1 + SN)
 *             (v_root too when that sum of priors is 0: the pass edge)
 *   qc_e    = q_e if N_e > 0 else v_mix;  lo, hi = min, max of qc;  qn_e = (qc_e - lo) / max(hi - lo, 1e-8)
 *   sigma_e = (c_visit + max_b N_b) * c_scale * qn_e
 *   score_e = (g_e + logit_e) + sigma_e        fp32, no contraction; the sums / min / max are wave reductions, not bit-pinned
 * Schedule: considered_visits(m, n) is the sequential-halving sequence of m considered actions and n simulations -- m <= 1:
 * 0, 1, .., n-1; else with L = ceil(log2 m) and k = m: emit max(1, n / (L k)) times the visit counts of the first k slots,
 * incrementing them after each emission, then k = max(2, k / 2), until n entries exist.
 * Selection at the root in simulation s >= 1 (simulation 0 only evaluates the root): t = considered_visits(min(max_considered,
 * ne), b - 1)[s - 1] with b = budget[g] when budgets are set, else `sims`; the edge is the argmax of score over the edges with
 * N_e == t, ties to the lower edge; over all edges when none has that count (a root visit taken back because the pool ran out;
 * counted by hive_search_gumbel_fallbacks).  s is the host's simulation counter, or clock + slot with per-game clocks.  No
 * Dirichlet noise is drawn for a Gumbel game.
 * Answer (hive_search_policy / _policy_where): action = argmax of score over the edges with N_e == max_b N_b (all edges before
 * the first visit), policy[act_e] = softmax_e(logit_e + sigma_e) over all ne edges, sum_n as ever; the pass edge answers -1
 * and writes nothing.  The "every W negative -> priors" fallback and the selfplay resampling of turns <= 6 do not apply to a
 * Gumbel game: the Gumbel draw is the exploration, and a quiet game is deterministic.
 *
 * c_visit = 50 and c_scale = 1 are the paper's values; they have not been tuned for this game. */
typedef struct HiveGumbelParams {
    int32_t max_considered; /* m: root actions sampled without replacement by Gumbel-top-m (16) */
    float c_visit;          /* 50 */
    float c_scale;          /* 1.0 */
    int32_t sims;           /* simulations per search while no budgets are set (the n + 1 of the schedule) */
} HiveGumbelParams;

/* prm == NULL (the default) switches the Gumbel root off.  where = DEVICE int8[games] the caller owns and the handle keeps the
 * pointer of, or NULL for every game: a game with where[g] == 0 is searched and answered exactly as without this call, bit for
 * bit.  Refused with HIVE_E_ARG: UCT mode (here, and hive_search_set_params to UCT while on); a handle with slots > 1 --
 * visits in flight would desynchronise the schedule; and hive_search_advance_roots returns HIVE_E_ARG while on -- a carried
 * root has no network value of its own and no fresh schedule. */
int hive_search_set_gumbel(HiveSearch *s, const HiveGumbelParams *prm, const int8_t *where);

/* The device's schedule function for tests: out_dev[i] = considered_visits(m, n)[i], i = 0 .. n-1 (device int32[n]). */
int hive_search_gumbel_schedule(int m, int n, int32_t *out_dev, void *stream);

/* The root quantities as the kernels compute them now, for tests and tools: g / logit / qhat (completed q) / improved =
 * float[games][HIVE_EDGE_CAP] each in edge order (any may be NULL), zero past the last edge and for a game without a tree.
 * HIVE_E_ARG while the Gumbel root is off. */
int hive_search_root_gumbel(HiveSearch *s, float *g, float *logit, float *qhat, float *improved);

/* int32[games]: root selections since create that found no edge at the scheduled visit count and took the best of all. */
int hive_search_gumbel_fallbacks(HiveSearch *s, int32_t *count);

/* ---- Gumbel selection below the root (section 5 of the same paper; mctx: gumbel_muzero_interior_action_selection).  Opt-in
 * on top of hive_search_set_gumbel.  Game g uses the rule iff it is a Gumbel game (hive_search_set_gumbel and its `where`),
 * on != 0 and (where == NULL or where[g] != 0); where = DEVICE int8[games] the caller owns and the handle keeps the pointer
 * of.  On every other game the call has no effect of any kind, bit for bit.  Accepted before or after
 * hive_search_set_gumbel; the default is off, and switching the Gumbel root off and on leaves this setting as it was.
 *
 * The rule.  It applies at a node x that the descent of such a game reaches at depth d >= 1 -- node 0 too, when a
 * transposition leads back to it; depth 0 stays the sequential-halving selection above.  x has edges e = 0 .. ne-1 with
 * P_e, N_e, W_e, and v_x = the value x was created with (hive_search_node_values).  logit_e, q_e, SN, v_mix, qc_e, qn_e and
 * sigma_e are the root's formulas above with v_x in the place of v_root and x's own max_b N_b.  There is no g_e: no noise is
 * drawn, for quiet and other games alike, and c_puct is not read.
 *   pi'_e   = softmax_e(logit_e + sigma_e) over all ne edges (the improved policy of hive_search_policy, at x)
 *   score_e = pi'_e - (float)N_e / (1.0f + (float)SN)        fp32, no contraction
 * The edge is the argmax of score, ties to the lower edge: the child whose visit share lags pi' most.  Unvisited children
 * are completed by v_mix, not by the q = 0 of PUCT.  A node with a single edge takes it as it is (the pass edge has P = 0).
 * Everything after the choice -- virtual loss, the move, the transposition lookup, expansion, pool exhaustion, the length
 * cap, finished games -- is hive_search_select's.  Gumbel games run on one slot (slots > 1 is refused by
 * hive_search_set_gumbel), so N_e holds no visit in flight of another simulation: the only virtual visits x can see are
 * this descent's own, when its line came through x before.
 * Unchanged: the answer at the root (action, improved policy, sum_n), hive_search_root_gumbel, budgets, per-game clocks, the
 * root's `where`, and every refusal of hive_search_set_gumbel. */
int hive_search_set_gumbel_interior(HiveSearch *s, int on, const int8_t *where);

/* ---- Proven wins and losses below the root (the MCTS-Solver rule: Winands, Bjornsson, Saito, "Monte-Carlo Tree Search
 * Solver", 2008).  Opt-in, PUCT mode, off by default; a game outside `where` is searched and answered bit for bit as without
 * the call.
 *
 * Status is a signed int8, 0 = unknown.  A NODE status s is taken from the side to move at the node: s > 0 that side wins,
 * s < 0 it loses, and |s| - 1 is the number of plies to the finished position under the proof.  An EDGE status e is taken
 * from the mover at the edge's parent, with the same meaning for the move.
 * What proves: only a finished game with a winner.  Such a node gets s = +1 when the side to move there is the winner, else
 * -1 (the winner rule that sets tv).  A finished game without a winner (both queens surrounded: the draw sentinel), the
 * length cap and a position without legal moves prove nothing: they keep status 0 and are averaged exactly as without the
 * option.
 * Propagation, in hive_search_backup after the value backup and only along the path of this simulation: c = the status of
 * the node where the path ended (a new or known finished game, or a node at which the descent stopped because it is proven).
 * While c != 0 and |c| < 127, for d = plen-1 .. 0 with P = path_node[d], k = path_edge[d]:
 *   e_status[P][k] = -sign(c) * (|c| + 1)
 *   s_P = the smallest positive e over all ne edges of P if any is positive (the fastest win), else -max|e| if every edge is
 *         negative (the longest resistance), else 0;  node_status[P] = s_P;  c = s_P
 * No early stop on "was already proven": the upper edges of this path may not know yet.  The pass edge is an edge like any
 * other.  An edge that was never backed up through an expanded child holds 0 and so blocks a loss proof.  Edge statuses are
 * written here and nowhere else: a position shared through the transposition table may be proven through one parent while
 * another parent's edge still says 0; that parent learns it when a descent next passes through it.  Statuses are path-local
 * until then, and every step is one the sequential player (solo_play.py, HivePlayer.solver) restates.
 * The length cap: the position key holds no turn number, so a node may be reached at a later turn than it was proven at.  A
 * status x HOLDS on a path whose current turn is T iff x != 0 and T + |x| - 1 <= max_game_length.  A status that does not
 * hold is treated as 0 by the two rules below; it stays stored.
 * Select: after the finished-game and the length-cap checks of hive_search_select, a node whose status holds ends the descent
 * (the root too: path length 0).  Such a descent is a known finished game: no leaf row, hive_search_leaf_need answers 0, the
 * value backed up is +1.0f or -1.0f by the sign, and it counts in bucket [3] of hive_search_leaf_histogram.  At a node that is
 * passed through, edges whose status holds and is negative are left out of the PUCT argmax unless all edges are such.  Noise,
 * virtual loss, collisions and pool exhaustion are unchanged.
 * Answer (hive_search_policy / _policy_where) at root turn T: root status holds and is > 0: the edge with the smallest positive
 * status that holds, ties to more visits, then to the lower edge; holds and is < 0: the edge with the largest |e|, same ties;
 * otherwise edges whose status holds and is negative are left out of the existing choice (argmax, the "every W negative ->
 * priors" fallback, the selfplay resampling) unless every edge is such.  A root with a holding status is not resampled.  The
 * policy row and sum_n are unchanged: the visit distribution as ever (a proven root ends descents at depth 0, so it collects
 * no further visits).
 * Not claimed: draws and the cap prove nothing; it is not combined with the Gumbel root (its halving schedule counts root
 * visits): HIVE_E_ARG from this call while hive_search_set_gumbel is on and from that call while this is on; HIVE_E_ARG in UCT
 * mode (here, and from hive_search_set_params to UCT while on).  Composes with slots > 1 (backups run slot after slot),
 * budgets, per-game clocks and hive_search_advance_roots, which moves both status arrays with the kept nodes and edges.
 *
 * on != 0 switches it on for the games with where[g] != 0 (DEVICE int8[games] the caller owns and the handle keeps the pointer
 * of; NULL = every game).  The first such call allocates node_status int8[games][max_nodes] and e_status
 * int8[games][max_nodes][HIVE_EDGE_CAP], and their twins in the second node pool, zeroed; from then on every node creation
 * writes its status and zeroes its edges' (nodes created earlier read 0). */
int hive_search_set_solver(HiveSearch *s, int on, const int8_t *where);

/* One game's statuses in hive_search_export_tree's layout: node = int8[max_nodes], edge = int8[max_nodes][HIVE_EDGE_CAP]
 * (either may be NULL).  Zeros before the first hive_search_set_solver. */
int hive_search_node_status(HiveSearch *s, int game, int8_t *node, int8_t *edge);

/* int8[games]: the stored status of node 0 (0 for a game without a tree). */
int hive_search_root_status(HiveSearch *s, int8_t *status);

/* int32[games][4] since create: [0] descents ended at a proven node, [1] nodes that became proven wins and [2] proven losses
 * by propagation (status 0 before), [3] answers taken from a proof. */
int hive_search_solver_stats(HiveSearch *s, int32_t *out);

/* The search's own noise generator, exposed for statistical tests: draw d (= 0 .. draws-1) is what the root of game id
 * `first_game + d` would get at (turn, sim 0, slot 0): eta ~ Dirichlet(alpha) over k <= HIVE_EDGE_CAP edges
 * (solo_play.py:322-323, np.random.dirichlet).  out = float[draws][k]; prior = float[k] or NULL:
 * out = (1 - eps) prior + eps eta (solo_play.py:323), or eta itself when prior is NULL. */
int hive_search_sample_noise(uint64_t seed, int64_t first_game, int turn, float alpha, int k, int draws, const float *prior,
                             float eps, float *out, void *stream);

/* ---- Arena: two networks play each other (woker/evaluation.py:40-111,128-310), both searched in ONE lock-step batch.
 *
 * A game is played by network A on one colour and network B on the other: a_white = int8[games], 1 = A is white.  A search
 * is the thinking of the side to move at its ROOT, so every leaf row of game g (rows are laid out slot * games + g, as
 * hive_search_select / hive_search_backup take them) belongs to network A iff a_white[g] == (root turn is odd); odd turn =
 * white to move (HiveBoard.turn).  All pointers are device pointers; stream = hipStream_t. */

/* need (int8[slots * games] of hive_search_leaf_need; NULL = all ones) split by owner:
 * need_a[r] = need[r] & owner_is_a, need_b[r] = need[r] & !owner_is_a.  rows_a / rows_b (either may be NULL): uint64
 * device counters, the number of rows flagged is ADDED to them. */
int hive_arena_split_launch(const HiveBoard *root_boards, const int8_t *a_white, const int8_t *need, int games, int slots,
                            int8_t *need_a, int8_t *need_b, uint64_t *rows_a, uint64_t *rows_b, void *stream);

/* Unequal sides: budget[g] (int32[games], for hive_search_set_budgets) = sims_a when A owns the search of game g -- the
 * ownership rule above -- else sims_b. */
int hive_arena_budget_launch(const HiveBoard *root_boards, const int8_t *a_white, int games, int sims_a, int sims_b,
                             int32_t *budget, void *stream);

/* In place: the rows B owns take B's prediction, p_a[r][0..1583] = p_b[r][..] and v_a[r] = v_b[r]; A's own rows are
 * untouched.  p = float[slots * games][1584], 16-byte aligned; v = float[slots * games]. */
int hive_arena_join_launch(const HiveBoard *root_boards, const int8_t *a_white, int games, int slots, float *p_a, float *v_a,
                           const float *p_b, const float *v_b, void *stream);

/* The uniformly random opening (evaluation.py:169,187 play random moves while turn <= 4): for every active game
 * (active = int8[n] or NULL) whose turn is <= opening_turns, action[g] = list[g][idx], or -1 (pass) when count[g] == 0;
 * idx = ((r >> 32) * count[g]) >> 32 with r = the first 64 bits of the search's counter-based generator keyed on
 * (seed, pair_id[g], turn, 0) and nothing else: both games of a pair, in any slot of any batch, get the same opening.
 * count = int32[n], list = int16[n][HIVE_LIST_CAP] ascending ids (hive_batch_legal), pair_id = int64[n].  Other entries of
 * action (int32[n]) are left alone. */
int hive_arena_opening_launch(const HiveBoard *boards, const int32_t *count, const int16_t *list, const int64_t *pair_id,
                              const int8_t *active, int n, uint64_t seed, int opening_turns, int32_t *action, void *stream);

/* Scores every active game (active = int8[n] or NULL) that is over or has reached the length cap (over / winner as
 * hive_batch_terminal: winner 1 white, 2 black, 0 none): result[g] (int8[n]) = 1 A won, 2 B won, 3 draw (both queens
 * surrounded), 4 length cap (turn >= max_game_length, game not over); 0 for every other game.  tally = int32[8], ADDED to:
 * [0] A wins as white [1] A wins as black [2] B wins as white [3] B wins as black [4] draws [5] length caps
 * [6] finished games [7] sum of their final turn numbers. */
int hive_arena_score_launch(const HiveBoard *boards, const int8_t *over, const int8_t *winner, const int8_t *active,
                            const int8_t *a_white, int n, int max_game_length, int8_t *result, int32_t *tally, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HIVE_SEARCH_H */
