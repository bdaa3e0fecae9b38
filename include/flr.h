/*
 * flr.h — C ABI of the MI355X-native federated-round engine (gfx950).
 *
 * Every entry point takes plain device pointers, element counts and a
 * hipStream_t passed as `void*` (NULL = the legacy default stream).  Nothing
 * here allocates: scratch space is caller-provided (query the size with the
 * matching *_workspace function).  Calls are stream-ordered and return as soon
 * as the work is enqueued.  Results are deterministic: fixed reduction order,
 * no float atomics, so 1/2/4/8-GPU runs give bit-identical outputs.
 *
 * Each function names the reference interface it replaces
 * (Shashank8834/multimodal-fl-security, paths relative to its repo root).
 *
 * Matrix convention ("client matrix"): X is K rows (clients, in global client
 * order) × P fp32 coordinates (the client's parameters flattened in
 * `model.parameters()` order, krum.py:55-57), row stride `ldx` elements.
 */
#ifndef FLR_H
#define FLR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define FLR_OK 0
#define FLR_ERR_ARG (-1)          /* invalid argument (shape, null pointer) */
#define FLR_ERR_HIP (-2)          /* a HIP runtime call or launch failed    */
#define FLR_ERR_UNSUPPORTED (-3)  /* shape outside what the kernels handle   */
#define FLR_ERR_WORKSPACE (-4)    /* workspace too small or misaligned       */
#define FLR_ERR_KRUM_N (-5)       /* n < 2f+3 (krum.py:153-157)             */

const char* flr_version(void);
/* "gfx950", or "gfx950 ablation" for the tools build (make ABLATION=1) that
 * adds the measured-slower and timing-only kernel forms. */
const char* flr_build_info(void);
/* The A/B switches (FLR_* names): the process environment's FLR_*
 * variables are read once, when the library loads; this sets (value NULL:
 * unsets) one afterwards, for an in-process A/B.  FLR_ERR_ARG unless the name
 * starts with FLR_. */
int flr_set_knob(const char* name, const char* value);
const char* flr_status_string(int status);
/* Last HIP error string recorded by a failing call on this thread. */
const char* flr_last_error(void);

/* ---- a9: Krum pairwise l2 ---------------------------------------------
 * Replaces KrumDefense._compute_distances (src/defenses/krum.py:73-99):
 *   D[i][j] = float32(||X_i - X_j||_2) stored as float64, D[i][i] = 0.
 * Engine: centred Gram matrix on MFMA (bf16 hi/lo split, fp32 accumulate),
 * fixed-order fp64 reduction of per-segment partials.  Any K >= 1.
 * Pairs the centring cannot condition (two rows close to each other but far
 * from the medoid pivot, e.g. a cluster of sign-flipped updates) are flagged
 * from the pivot sample and recomputed from exact fp32 differences (up to 128
 * such rows per call: every row at K <= 128).  More flagged rows than that
 * (K > 128 only) makes EVERY D entry NaN, the diagonal included — the marker
 * callers test (D[0][0] is NaN only then; NaN client rows leave the diagonal
 * 0): a loud failure, never a silently inaccurate distance.
 */
size_t flr_pairwise_l2_workspace(int64_t K, int64_t P);
int flr_pairwise_l2(const float* X, int64_t K, int64_t P, int64_t ldx,
                    double* D, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Same, recording two caller-created hipEvent_t around the main MFMA kernel
 * launch(es) on `stream` (for live per-kernel timing); either may be NULL. */
int flr_pairwise_l2_ex(const float* X, int64_t K, int64_t P, int64_t ldx,
                       double* D, void* workspace, size_t workspace_bytes,
                       void* stream, void* ev_begin, void* ev_end);

/* Coordinate-sharded form of the same computation (the exchange mode where
 * GPU g holds ALL K clients but only a contiguous range of coordinates, see
 * DESIGN.md §2).  The full chunks (64 coordinates) of the vector are cut into
 * FLR_PW_SLICES canonical slices; flr_pairwise_l2 itself runs on exactly these
 * slices, so composing the phases below over any split of the slices gives
 * D bit-identical to flr_pairwise_l2 on the whole matrix:
 *   1. flr_pairwise_sample on every holder, then an exact SUM of the [K][S]
 *      samples (the positions a holder does not own are written as 0);
 *   2. flr_pairwise_pivot on the combined sample (replicated) -> the pivot
 *      record, flr_pairwise_pivot_len() int32 (pivot, refined-row count, rows);
 *   3. flr_pairwise_gram_slices for the holder's slices [q0, q1): X's column
 *      0 is the first coordinate of slice q0 (chunk flr_pw_slice_chunks(q0));
 *      gsum [q1-q0][flr_pairwise_gsum_len(K)] fp64;
 *   4. flr_pairwise_tail on the holder of the coordinates past the last full
 *      chunk (everyone else: p0 == p1, writes zeros), then an exact SUM;
 *   5. gather the gsum blocks of all slices in slice order ->
 *      [FLR_PW_SLICES][gsum_len]; flr_pairwise_finish -> D.
 * P is always the WHOLE vector's length. */
#define FLR_PW_SLICES 8
int flr_pw_slice_chunks(int64_t P, int64_t q, int64_t* chunk_begin, int64_t* chunk_end);
int64_t flr_pairwise_sample_len(int64_t P);
size_t flr_pairwise_gsum_len(int64_t K);
int64_t flr_pairwise_pivot_len(void);
size_t flr_pairwise_sliced_workspace(int64_t K, int64_t P, int64_t nslices);
int flr_pairwise_sample(const float* X, int64_t K, int64_t ldx, int64_t P, int64_t chunk0,
                        int64_t chunk1, float* Xs, void* stream);
int flr_pairwise_pivot(const float* Xs, int64_t K, int64_t P, int* pivot, void* workspace,
                       size_t workspace_bytes, void* stream);
int flr_pairwise_gram_slices(const float* X, int64_t K, int64_t ldx, int64_t P, int64_t q0,
                             int64_t q1, const int* pivot, double* gsum, void* workspace,
                             size_t workspace_bytes, void* stream, void* ev_begin,
                             void* ev_end);
int flr_pairwise_tail(const float* X, int64_t K, int64_t ldx, int64_t p0, int64_t p1,
                      double* tail, void* stream);
int flr_pairwise_finish(const double* gsum, const double* tail, int64_t K, double* D,
                        void* stream);

/* Reference-exact variant (pairwise_method="reference"):
 * D[i][j] bit-identical to the reference's fp32 torch.norm(flat_i - flat_j)
 * .item() (krum.py:89-97) — per pair, 8 fp32 chains of sequential
 * fma(d, d, chain) over every 8th coordinate d = fl(x_i - x_j), the chains
 * summed 0..7 in order, the P mod 8 tail added in order (a first group of 4
 * as separate multiply + add, the last 0..3 as fma), correctly rounded
 * sqrt_f32 (tail probed in tools/diag_norm_host.py;
 * oracle/norm_ref.c; the same bits under torch's AVX2 and AVX512 dispatch,
 * tests/test_oracle.py test_norm_ref_model_cpu_capability).  X in the reference's coordinate order (parameters()
 * order); rows 16-B aligned and ldx % 4 == 0 (else FLR_ERR_ARG).
 * Workspace (256-B aligned): flr_pairwise_l2_reference_workspace(K, P) bytes
 * — the chains' running sums plus one chain-major copy of a coordinate segment
 * (at most 8 GiB; a smaller workspace runs more, shorter segments, the same
 * result; segments hold whole multiples of 512 chain steps, zero-filled past
 * the last, plus 4 KB of prefetch slack: below K x 16 KiB + 4 KiB past the
 * sums, FLR_ERR_WORKSPACE).  part / nparts: this call computes the pairs of tile range
 * [part * T / nparts, (part + 1) * T / nparts), T =
 * flr_pairwise_l2_reference_tiles(K), and writes 0 for every other pair: the
 * nparts results summed (exact: one non-zero term per pair) are the whole D.
 * VALU-issue bound: each pair's 8 chains run the whole vector sequentially. */
size_t flr_pairwise_l2_reference_workspace(int64_t K, int64_t P);
int flr_pairwise_l2_reference_tiles(int64_t K);
int flr_pairwise_l2_reference(const float* X, int64_t K, int64_t P, int64_t ldx,
                              double* D, void* ws, size_t ws_bytes, int64_t part,
                              int64_t nparts, void* stream);
/* The same over a training-order client matrix: the ntaps blocks taps[4b ..
 * 4b+3] = {off, Cout, Cin, KK} (ascending, disjoint, inside [0, P)) hold a
 * convolution weight stored tap-major, column off + (t * Cin + ci) * Cout + co
 * for reference coordinate off + (co * Cin + ci) * KK + t (torch's
 * [Cout][Cin][kh][kw]); every other column is its own coordinate.  The
 * trainers' layout (flr_resnet_gru_reorder), so a round's matrix goes in as
 * written, no torch-order copy; ntaps = 0 is flr_pairwise_l2_reference. */
int flr_pairwise_l2_reference_tap(const float* X, int64_t K, int64_t P, int64_t ldx,
                                  const int64_t* taps, int64_t ntaps, double* D, void* ws,
                                  size_t ws_bytes, int64_t part, int64_t nparts, void* stream);
/* The same with dead taps: dead[b] bit t set = tap t of block b is not in X
 * (FLR_TC_DEFER_DEAD): its slab is read from gdead at the same training-order
 * offset, negated on rows k < nneg — the values flr_resnet_gru_fill_dead
 * writes, so D is bit-identical to the call on the filled X.  No dead column
 * may lie in the last P mod 8 (read from X): FLR_ERR_ARG.
 * A 3 x 3 block at off % 8 == 0 with Cout Cin % 8 == 0 whose live taps are the
 * centre alone (mask 0x1EF) or taps 4, 5, 7, 8 (mask 0x04F) runs as a dead
 * region (part 0 of 1): only its live coordinates are
 * rewritten, its dead ones come from one shared stream of g + g that the pairs
 * with exactly one negated row add in the chain's order, and the other pairs
 * skip them (fl(g - g) = +0; a dead value of g that is not finite makes those
 * pairs NaN, as on the filled X).  Any other block is expanded from gdead as
 * before; the knob FLR_REF_DEAD_SKIP=0 (flr_set_knob) expands every block.  The
 * same bits either way. */
int flr_pairwise_l2_reference_tap_dead(const float* X, int64_t K, int64_t P, int64_t ldx,
                                       const int64_t* taps, int64_t ntaps, const uint64_t* dead,
                                       const float* gdead, int64_t nneg, double* D, void* ws,
                                       size_t ws_bytes, int64_t part, int64_t nparts, void* stream);
/* The same split over coordinate ranges held by different ranks (the
 * coordinate-sharded exchange): each range continues the chains where the
 * previous range left them.  _partial: `steps` chain steps of X (coordinates
 * 0 .. 8 steps - 1 of each row; a range starting at a multiple of 8 reference
 * coordinates) added to the running chain sums held in ws's first 8 K^2 floats
 * (first: start from 0; otherwise the previous range's ws sums, copied in);
 * ws as for flr_pairwise_l2_reference_workspace(K, 8 steps).  _finish: D from
 * the chain sums (chains = 0: none) and the last P mod 8 coordinates (Xtail,
 * ntail <= 7).  Each step is the same fp32 operation in the same order as in
 * the one-call form, so D is bit-identical to it. */
int flr_pairwise_l2_reference_partial(const float* X, int64_t K, int64_t steps, int64_t ldx,
                                      int first, void* ws, size_t ws_bytes, void* stream);
int flr_pairwise_l2_reference_finish(const float* Xtail, int64_t K, int64_t ntail, int64_t ldx,
                                     int chains, const void* ws, double* D, void* stream);
/* The same partial chains over a TRAINING-ORDER coordinate slice (a rank of
 * a training-order round at G > 1): taps {off, Cout, Cin, KK} name the
 * tap-major blocks inside the slice (offsets from X, each wholly inside
 * [0, 8 steps)), as flr_pairwise_l2_reference_tap; the slice must hold whole
 * blocks (the round engine aligns its rank boundaries to them). */
int flr_pairwise_l2_reference_partial_tap(const float* X, int64_t K, int64_t steps, int64_t ldx,
                                          const int64_t* taps, int64_t ntaps, int first, void* ws,
                                          size_t ws_bytes, void* stream);

/* Direct-difference VALU variant (same contract, exact fp32 differences);
 * a slower second implementation used to cross-check the MFMA path. */
size_t flr_pairwise_l2_direct_workspace(int64_t K, int64_t P);
int flr_pairwise_l2_direct(const float* X, int64_t K, int64_t P, int64_t ldx,
                           double* D, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- a10: Krum score + selection --------------------------------------
 * Replaces KrumDefense._krum_score + the argsort in aggregate
 * (src/defenses/krum.py:101-131, 149-176):
 *   m = K - f - 2; scores[i] = numpy-pairwise-sum(sort(D[i])[1 : m+1]);
 *   order = argsort(scores) (ties broken by lower client index).
 * NaN in numpy's order: after every value in the row sort and in the argsort
 * (a client whose update is NaN gets a NaN score and the last ranks).
 * D: device fp64 K×K (row-major, ld = K). scores: device fp64 [K];
 * order: device int32 [K].  Returns FLR_ERR_KRUM_N if K < 2f+3.
 */
int flr_krum_select(const double* D, int64_t K, int64_t f, double* scores,
                    int32_t* order, void* stream);

/* ---- a11: Multi-Krum mean ---------------------------------------------
 * Replaces the Multi-Krum average (src/defenses/krum.py:182-192):
 *   out = (((0 + X[rows[0]]) + X[rows[1]]) + ...) / divisor   (fp32, in order)
 * rows: device int32 [m] (e.g. the first m entries of `order`); divisor is
 * the reference's multi_k (== m unless multi_k > K).
 * Precondition: every rows[i] in [0, K).  The indices are device-resident, so
 * this is not checked on the host; an out-of-range index is clamped into range
 * on the device (no out-of-bounds read) and the result is then unspecified.
 */
int flr_rows_mean(const float* X, int64_t K, int64_t P, int64_t ldx,
                  const int32_t* rows, int64_t m, int64_t divisor, float* out,
                  void* stream);
/* The same over a training-order matrix whose dead-tap ranges [dead_off[r],
 * + dead_n[r]) are not written (the round engine's FLR_DEFER_DEAD=2): row k's
 * value there is gdead's, negated for k < nneg, summed in the same order —
 * bit-identical to flr_rows_mean over the filled rows; X's dead ranges are not
 * read (the float4 groups wholly inside them).  16-B aligned rows and out. */
int flr_rows_mean_dead(const float* X, int64_t K, int64_t P, int64_t ldx, const int32_t* rows,
                       int64_t m, int64_t divisor, const int64_t* dead_off, const int64_t* dead_n,
                       int64_t ndead, const float* gdead, int64_t nneg, float* out, void* stream);

/* ---- a14: FedAvg -------------------------------------------------------
 * Replaces NoDefense.aggregate (src/defenses/base_defense.py:80-97) and the
 * inline FedAvg of experiments/run_experiments.py:246-254:
 *   out = (sum_i fl(n_i * X_i)) / sum_i n_i     (fp32, client order)
 * num_examples: device int64 [K].
 */
int flr_fedavg(const float* X, int64_t K, int64_t P, int64_t ldx,
               const int64_t* num_examples, float* out, void* stream);

/* ---- a12: coordinate-wise trimmed mean ---------------------------------
 * Replaces TrimmedMeanDefense.aggregate (src/defenses/trimmed_mean.py:48-90)
 * for one fixed t (= max(1, int(K*trim_ratio)), computed by the caller):
 *   out[p] = mean(sort(X[:,p])[t : K-t])   (torch's cascade-sum order)
 * Requires K - 2t >= 1 (the caller falls back to the median otherwise).
 */
int flr_trimmed_mean(const float* X, int64_t K, int64_t P, int64_t ldx,
                     int64_t t, float* out, void* stream);

/* ---- a13: coordinate-wise lower median ---------------------------------
 * Replaces MedianDefense.aggregate / _coordinate_wise_median
 * (src/defenses/trimmed_mean.py:92-103, 141-166): torch.median(dim=0)[0]
 * = sort(X[:,p])[(K-1)/2]. Bit-exact (selection, no arithmetic).
 */
int flr_median_lower(const float* X, int64_t K, int64_t P, int64_t ldx,
                     float* out, void* stream);

/* The same two order statistics over the row subset rows[0..m) of X (device
 * int32 indices, m <= K <= 512): the coordinate-wise trimmed mean of the
 * Multi-Krum selection ("Krum + trimmed-mean", BASELINE.json configs[4]).
 * Precondition as flr_rows_mean: rows[i] in [0, K) (out-of-range indices are
 * clamped on the device, never read out of bounds; the result is unspecified). */
int flr_trimmed_mean_rows(const float* X, int64_t K, int64_t P, int64_t ldx, const int32_t* rows, int64_t m,
                          int64_t t, float* out, void* stream);
int flr_median_lower_rows(const float* X, int64_t K, int64_t P, int64_t ldx, const int32_t* rows, int64_t m,
                          float* out, void* stream);

/* ---- Bulyan (El Mhamdi, Guerraoui, Rouault, ICML 2018) ------------------
 * Stage 2, the median-window mean over the m rows rows[0..m) of X (rows NULL:
 * rows 0..m-1; m = K is the whole matrix), m <= 128.  Per coordinate: sort
 * ascending into s[0..m), med = s[(m-1)/2] (the lower median); take the beta
 * ranks with the smallest fp32 |s[r] - med|, equal distances to the smaller
 * value — a window [lo, lo+beta) around the median rank; sum it in rank order
 * (sequential fp32 adds from 0.f, no FMA) and divide once by beta.  beta = m is
 * the mean of all rows in rank order, beta = 1 the lower median.  NaNs sort
 * last; the result is NaN when the column holds more than m - beta of them or
 * the median rank is one.  Columns holding +-inf: unspecified, read in bounds.
 * FLR_ERR_ARG: null X / out, m < 1, m > K, beta < 1, beta > m, ldx < P;
 * FLR_ERR_UNSUPPORTED: m > 128.  rows as flr_rows_mean (clamped on the device). */
int flr_median_window_mean_rows(const float* X, int64_t K, int64_t P, int64_t ldx, const int32_t* rows,
                                int64_t m, int64_t beta, float* out, void* stream);

/* Stage 1, the iterated Krum selection on the fp64 distance matrix D (device,
 * K×K row-major), all on the device, no host synchronisation.  alive = every
 * client; theta times, with n_r clients alive: m_r = min(n_r - 1, max(1, n_r -
 * f - 2)); an alive client's score is the numpy pairwise sum of ranks 1..m_r of
 * its sorted distances to the alive clients (Krum's rule on the sub-matrix);
 * the smallest score is picked (exact ties: the lowest client index; NaN scores
 * last) and leaves the alive set.
 * scores: device fp64 [K], the first iteration's scores (flr_krum_select's, bit
 * for bit, where that call is defined).  picked: device int32 [K], the theta
 * picks in pick order, then the unpicked clients in ascending index.  Every
 * slot of both is written on every call.
 * FLR_ERR_ARG: null pointer, K < 1, f < 0, theta outside [1, K];
 * FLR_ERR_UNSUPPORTED: K > 1024; FLR_ERR_WORKSPACE: workspace null or smaller
 * than flr_krum_select_iter_workspace(K) (0 for K <= 0).  Bulyan's n >= 4f + 3
 * is the caller's rule. */
size_t flr_krum_select_iter_workspace(int64_t K);
int flr_krum_select_iter(const double* D, int64_t K, int64_t f, int64_t theta, double* scores,
                         int32_t* picked, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a16: colluding model-poisoning attacks (ALIE, IPM) -----------------
 * ALIE (Baruch, Baruch, Goldberg, NeurIPS 2019) and IPM with a benign mean
 * (Xie, Koyejo, Gupta, UAI 2019; InnerProductManipulationAttack.poison_update,
 * src/attacks/model_poisoning.py, the branch next to the sign flip), in place
 * on the client matrix: rows [0, nmal) are the attackers and are overwritten,
 * all with the same vector; rows [nmal, K) are benign and only read; columns
 * [P, ldx) are never touched.  Per coordinate, nb = K - nmal, the benign rows in
 * ascending row order, every operation a separately rounded fp32 op (no FMA):
 *   s = sequential adds of x_k from 0.f;           mu = s / (float)nb
 *   q = sequential adds of (x_k - mu)*(x_k - mu) from 0.f
 *   sigma = sqrt(q / (float)nb)     (population deviation, correctly rounded)
 *   FLR_COLLUDE_ALIE: out = mu - param * sigma;  FLR_COLLUDE_IPM: out = -(param * mu)
 * so a torch CPU loop over the rows gives the same bits.  NaN and inf follow
 * IEEE: a NaN in a benign row makes that coordinate of the attackers' rows NaN
 * and no other.  mean_out / std_out: optional device fp32 [P] (NULL: not
 * written), mu and sigma; in IPM mode sigma is computed only for std_out.
 * Coordinate-wise: any column range of X (same ldx) gives that range of the
 * whole-matrix result.  Any K; no workspace.
 * FLR_ERR_ARG: null X, K < 2, nmal < 1, nmal >= K, P < 1, ldx < P, mode outside
 * {0, 1}; nothing is written then. */
#define FLR_COLLUDE_ALIE 0   /* out = mu - param * sigma   (param = z)       */
#define FLR_COLLUDE_IPM  1   /* out = -(param * mu)        (param = epsilon) */
int flr_collude_rows(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal,
                     int mode, float param, float* mean_out, float* std_out,
                     void* stream);

/* ---- Min-Max / Min-Sum colluding attacks (Shejwalkar, Houmansadr, NDSS 2021)
 * "Manipulating the Byzantine": aggregator-agnostic; no reference counterpart.
 * In place on the client matrix, as flr_collude_rows: rows [0, nmal) are the
 * attackers and are overwritten, all with the same vector m = mu + gamma * p;
 * rows [nmal, K) are benign and only read, nb = K - nmal; columns [P, ldx) are
 * never touched.  The rows are model weights; `global` (device fp32 [P]) is the
 * model the clients started from.  gamma is the largest strength >= 0 with
 *   FLR_MINMAX_MAX:  max_i ||m - x_i||^2 <= R2 = max_ij ||x_i - x_j||^2
 *   FLR_MINMAX_SUM:  sum_i ||m - x_i||^2 <= S  = max_i sum_j ||x_i - x_j||^2
 * over the benign rows, solved in closed form (the paper halves an interval,
 * one pass over the matrix per probe).  The whole call is enqueued on the
 * stream, no host synchronisation.  Stages, op for op:
 *   1. mu, sigma: flr_collude_rows' mean_out / std_out (its arithmetic, its
 *      bits), no row written.
 *   2. D: flr_pairwise_l2 (the Gram engine) on the benign rows, nb x nb fp64
 *      holding float32-rounded distances.  R2 and S are DEFINED from it, in fp64:
 *        R2 = max_ij D[i][j]*D[i][j];   S = max_i (sequential sum over j = 0..nb-1
 *        of D[i][j]*D[i][j], from 0.0);   a NaN term makes the maximum NaN.
 *   3. the perturbation, per coordinate, fp32:
 *        FLR_PERTURB_STD:   p = -sigma
 *        FLR_PERTURB_SIGN:  t = mu - g;  p = -sign(t), sign(0) = 0, sign(NaN) = NaN
 *        FLR_PERTURB_UNIT:  p = -(mu - g), NOT normalised: only p's direction
 *                           matters for the rows, and gamma is relative to this
 *                           p — gamma * sqrt(c) is the paper's unit-vector gamma.
 *      and the statistics, d_ik = fl32(mu_k - x_ik):
 *        a_i = sum_k d_ik*d_ik    b_i = sum_k p_k*d_ik    c = sum_k p_k*p_k
 *      each product exact in fp64, each sum a fixed-order fp64 sum whose order is
 *      the kernel's own (a function of K, P, ldx and the pointers' 16-B alignment
 *      alone: run-to-run identical bits, no float atomics), so they are accurate
 *      to about P * 2^-53 relative, not bit-defined.  X is read once for both.
 *   4. gamma, fp64, every operation correctly rounded, in the order written
 *      (bit-defined given a, b, c, R2, S):
 *        any of a_i, b_i, c, R2, S NaN:   gamma = NaN
 *        else c == 0:                     gamma = 0      (e.g. nb = 1 with STD)
 *        else FLR_MINMAX_MAX:  h_i = R2 - a_i, h_i < 0 replaced by 0 (a_i <= R2
 *                                 mathematically: the mean is in the benign hull)
 *                              gamma_i = (sqrt(b_i*b_i + c*h_i) - b_i) / c
 *                              gamma = min_i gamma_i; a NaN gamma_i (inf - inf in
 *                                 h_i) makes it NaN (numpy's min)
 *        else FLR_MINMAX_SUM:  A = sequential sum of a_i, Bs = of b_i, from 0.0
 *                              h = S - A, h < 0 replaced by 0;  n = (double)nb * c
 *                              gamma = (sqrt(Bs*Bs + n*h) - Bs) / n
 *   5. the rows (bit-defined given mu, p, gamma), two separately rounded fp32
 *      ops as in flr_collude_rows:   out = mu + (float)gamma * p
 *      gamma NaN: nothing is written — one NaN in a benign row does not become
 *      NaN in every attacker row; the returned gamma says so.  (The Gram
 *      engine's all-NaN marker at nb > 128, see flr_pairwise_l2, ends the same way.)
 * gamma_out: optional device fp64 scalar.  stats_out: optional device fp64
 * [2*nb + 4]: a_i [nb], b_i [nb], c, R2, S, the bound used (R2 or S).
 * Workspace: flr_minmax_workspace(K, P, nmal) bytes (0 for arguments the call
 * rejects), 256-byte aligned; it includes flr_pairwise_l2's.  After the call
 * its first P floats hold mu and the P floats at byte offset
 * (4*P + 255) / 256 * 256 hold sigma.
 * Bytes moved: 3 * nb * P * 4 read (mean, Gram, statistics) + nmal * P * 4 written.
 * FLR_ERR_ARG: null X, K < 2, nmal < 1, nmal >= K, P < 1, ldx < P, objective or
 * perturb outside their values, global NULL unless FLR_PERTURB_STD.
 * FLR_ERR_WORKSPACE: workspace null, too small or not 256-byte aligned.
 * FLR_ERR_UNSUPPORTED: nb > 1024, flr_pairwise_l2's row limit (the one-workgroup
 * solve alone would carry 4096).  Nothing is written on an error.
 * nb = 1 is legal: R2 = S = 0, a_0 = 0, gamma = 0, the rows become mu. */
#define FLR_MINMAX_MAX 0
#define FLR_MINMAX_SUM 1
#define FLR_PERTURB_STD 0
#define FLR_PERTURB_SIGN 1
#define FLR_PERTURB_UNIT 2
size_t flr_minmax_workspace(int64_t K, int64_t P, int64_t nmal);
int flr_minmax_rows(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal,
                    int objective, int perturb, const float* global,
                    double* gamma_out, double* stats_out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- model replacement: the scaled backdoor (Bagdasaryan et al., AISTATS 2020)
 * "How To Backdoor Federated Learning": the attackers (rows 0..f-1, trained on
 * triggered data) boost their update so that it survives the average,
 *   x_i <- g + gamma_i * (x_i - g),      g the model the round trained from,
 * and shrink it back under the bound the server enforces (Sun et al. 2019, "Can
 * You Really Backdoor Federated Learning?"; Wang et al., NeurIPS 2020; the
 * "constrain" half of constrain-and-scale).  No reference counterpart.  Two
 * calls, each enqueued on the stream with no host synchronisation; nothing is
 * written on an error.
 *
 * flr_replace_strength: gamma_i of the f attackers from the round's own matrix.
 * One workgroup, a lane per client; all arithmetic fp64, every operation rounded
 * on its own (no FMA), only + - * / sqrt, in this order.
 *   e_j: norms[j] = ||x_j - g|| (flr_row_norms with the center g); in distance
 *     mode norms may be NULL, then e_j = sqrt(G_jj).
 *   G: the centered Gram matrix flr_rows_gram(X, center = g), G_jk = <x_j - g,
 *     x_k - g>; read in distance mode only (NULL otherwise), taken as symmetric
 *     (the kernel reads G_ji for G_ij).
 *   The benign rows are f..K-1, nb = K - f of them.
 *   FLR_REPLACE_NONE: gamma_i = boost, status 0; norms and G are not read.
 *   FLR_REPLACE_NORM: gamma_i = min(boost, rho * B / e_i), B a statistic of the
 *     benign e_j:
 *       FLR_REPLACE_MEDIAN  numpy's median: the sorted values' middle one, or
 *                           (lo + hi) / 2 of the two middle ones
 *       FLR_REPLACE_MAX     the largest
 *       FLR_REPLACE_MEAN    ((e_f + e_f+1) + ...) + e_K-1, rows ascending, / nb
 *     a NaN among the benign e_j makes B NaN (+inf is a value like any other).
 *       bound = rho * B
 *       e_i == 0:                gamma_i = boost            status 0
 *       boost * e_i <= bound:    gamma_i = boost            status 0
 *       else:                    gamma_i = bound / e_i      status 1
 *   FLR_REPLACE_DISTANCE: the largest gamma_i <= boost with
 *     ||g + gamma_i (x_i - g) - x_j|| <= rho * max_{j,k benign} ||x_j - x_k|| for
 *     every benign j — the Min-Max criterion on each attacker's own direction.
 *       D2 = max(0, max_{j<k benign} ((G_jj + G_kk) - 2 * G_jk)), a NaN term kept
 *       b2 = (rho * rho) * D2                                 (B = D2 here)
 *       per attacker i, a = G_ii, and benign j, b = G_ij, c = G_jj - b2:
 *         disc = b * b - a * c            (two products, one subtraction)
 *         gamma_ij = (b + sqrt(max(0, disc))) / a
 *           (the larger root of a t^2 - 2 b t + c = 0; disc < 0: no t meets row
 *           j's bound, gamma_ij = b / a is the point closest to x_j)
 *       m = min_j gamma_ij, a NaN once seen kept
 *       gamma_i = min(boost, max(0, m))
 *       status 2 when some disc < 0 or m < 0 (no gamma >= 0 meets every bound),
 *       else 1 when gamma_i < boost, else 0.   a == 0: gamma_i = boost, status 0.
 *   Not finite: B not finite sets every gamma_i = 1, every status 3 and bit 0 of
 *     flags.  Otherwise an attacker with e_i not finite (distance mode: G_ii not
 *     finite too) or a NaN gamma_i gets gamma_i = 1, status 3, and sets bit 1.
 *   gamma32_i = (float)gamma64_i.
 * gamma64: device fp64 [f]; gamma32: device fp32 [f]; status: device int32 [f]
 * (0 boost-limited, 1 bound-limited, 2 infeasible: the closest point taken, 3 left
 * alone: gamma = 1); flags: device int32 [1].  Bytes: norms once; distance mode
 * reads the benign block of G once and the attackers' columns once (L2).
 * FLR_ERR_ARG: null gamma64, gamma32, status or flags; norms NULL in norm mode; G
 * NULL in distance mode; f < 1; f >= K; boost or rho not a finite number > 0; mode
 * or stat outside their values; distance mode with K - f < 2.
 * FLR_ERR_UNSUPPORTED: K > 1024.
 *
 * flr_scale_rows_from, in place, rows i < n: three separately rounded fp32
 * operations per element (no FMA),
 *   X_ip = fl(c_p + fl(fl(X_ip - c_p) * gamma_i))
 * A row with gamma_i == 1 or a NaN gamma_i is neither read nor written (boost = 1
 * is the plain backdoor bit for bit).  Rows >= n and columns [P, ldx) are never
 * touched.  center: device fp32 [P], not inside X; gamma32: device fp32 [n].  A
 * workgroup owns 256 lanes of one row, a lane one float4 of coordinates (or one
 * coordinate: X or center not 16-byte aligned, or ldx % 4 != 0; the same bits).
 * n == 0: FLR_OK, nothing done.
 * Bytes moved: 2 * (rows with gamma != 1) * P * 4 + P * 4 (the center is read once
 * per scaled row; past the first the caches serve it).
 * FLR_ERR_ARG: null X, center or gamma32; K < 1; P < 1; ldx < P; n < 0; n > K.
 * FLR_ERR_UNSUPPORTED: n > 65535. */
#define FLR_REPLACE_NONE 0
#define FLR_REPLACE_NORM 1
#define FLR_REPLACE_DISTANCE 2
#define FLR_REPLACE_MEDIAN 0
#define FLR_REPLACE_MAX 1
#define FLR_REPLACE_MEAN 2
int flr_replace_strength(const double* norms, const double* G, int64_t K, int64_t f,
                         double boost, int mode, int stat, double rho, double* gamma64,
                         float* gamma32, int32_t* status, int32_t* flags, void* stream);
int flr_scale_rows_from(float* X, int64_t K, int64_t P, int64_t ldx, const float* center,
                        const float* gamma32 /* device [n] */, int64_t n, void* stream);

/* ---- Fang et al.'s full-knowledge attacks on Krum and on the trimmed mean -----
 * Fang, Cao, Jia, Gong, "Local Model Poisoning Attacks to Byzantine-Robust
 * Federated Learning", USENIX Security 2020: the attacks written against one
 * aggregation rule each, the baseline Min-Max / Min-Sum are measured against.  No
 * reference counterpart.  In place on the client matrix, as flr_collude_rows:
 * rows [0, nmal) are the attackers and are overwritten, rows [nmal, K) are benign
 * and only read, nb = K - nmal; columns [P, ldx) are never touched.  The rows are
 * model weights; `global` (device fp32 [P]) is the model g the round trained
 * from.  Every call is enqueued on the stream, no host synchronisation; nothing
 * is written on an error.
 *
 * The directed deviation, shared by both: mu is flr_collude_rows' mean_out (its
 * arithmetic, its bits) and, per coordinate, fp32,
 *   t = fl(mu - g);  s = sign(t), sign(0) = 0, sign(NaN) = NaN
 * the FLR_PERTURB_SIGN convention.  (The paper maps 0 to -1; here a coordinate
 * the benign clients did not move is not attacked.)
 *
 * flr_fang_krum_rows, the Krum attack: every attacker submits m = g - lambda * s,
 * all nmal rows identical (the paper's epsilon-ball around the first is dropped,
 * as in the authors' later code), lambda the largest of lambda0 * 2^-t, t = 0, 1,
 * ..., for which Krum picks an attacker's row — flr_krum_select's rule: the score
 * is the sum of the K - f - 2 smallest distances to the others, the smallest
 * score wins, ties to the lower index (the attackers have the lower indices).
 * The paper probes each lambda with a Krum over the attacked matrix; here the
 * probe is closed: with u_i = x_i - g over the benign rows, G_ij = <u_i, u_j>,
 * b_i = <s, u_i>, c = <s, s>,  ||m - x_i||^2 = G_ii + 2 lambda b_i + lambda^2 c,
 * and the benign rows' mutual distances do not depend on lambda.  Stages:
 *   1. mu: as above, no row written.
 *   2. G: flr_rows_gram on the benign rows with center g, nb x nb fp64.
 *   3. b_i = sum_k s_k * fl(x_ik - g_k), c = sum_k s_k * s_k: each product exact
 *      in fp64, each sum a fixed-order fp64 sum whose order is the kernel's own (a
 *      function of K, P, ldx and the pointers' 16-B alignment alone: run-to-run
 *      identical bits, no float atomics), accurate to about P * 2^-53 relative,
 *      not bit-defined.  The benign rows are read once; s is stored beside mu.
 *   4. flr_fang_krum_strength (a call of its own: G, b, c device inputs).  All
 *      arithmetic fp64, every operation rounded on its own (no FMA), only + - * /
 *      sqrt, in this order; max0(x) is 0 for x < 0, else x (a NaN stays):
 *        m = K - f - 2;  na = K - 2f - 1;  e_i = G_ii             (f = nmal)
 *        D_ij = sqrt(max0((e_i + e_j) - 2 * G_ij))  for j != i
 *        r_i = those nb - 1 values in ascending order, NaN last (a kernel of a
 *          workgroup per row, into the workspace)
 *        then one workgroup, a lane per benign row:
 *        T_i = sequential sum from 0.0 of r_i[0 .. m-1];  T = min_i T_i, a NaN kept
 *        E = max_i sqrt(e_i), a NaN kept;  rc = sqrt(c)
 *        any NaN among e_i, b_i, c, T:  lambda = NaN, status 3
 *        else c == 0:                   lambda = 0,   status 2   (g == mu: no direction)
 *        else lambda0 = T / ((double)na * rc) + E / rc
 *          (the paper's Theorem 1 with its m -> K, c -> f, and sqrt(d) -> rc
 *          because s may hold zeros);  lambda0 not finite: lambda = NaN, status 3
 *        else for t = 0, 1, ...: lambda = lambda0 halved t times
 *          lambda <= threshold:  stop, status 1, this lambda (the search failed;
 *            with f = 1 it usually does, as the paper says: one crafted model has
 *            no zero-distance companion)
 *          d_i = sqrt(max0((e_i + (2 * lambda) * b_i) + (lambda * lambda) * c))
 *          S_att = sequential sum from 0.0, ascending, of the na smallest d_i (an
 *            attacker's score: its f - 1 companions are at distance 0)
 *          S_i = sequential sum from 0.0, ascending, of the m smallest of the
 *            multiset r_i and f copies of d_i (NaN last)
 *          S_min = min_i S_i, a NaN kept
 *          S_att <= S_min:  stop, status 0, this lambda
 *      lambda64: device fp64 [1]; lambda32 = (float)lambda64: device fp32 [1];
 *      info: device int32 [2], status (0 found, 1 threshold reached, 2 no
 *      direction, 3 not finite) and t (0 for status 2 and 3); stats_out: optional
 *      device fp64 [5]: lambda0, T, E, the last probe's S_att and S_min (NaN where
 *      not computed).  G: device fp64 nb x nb (the benign rows alone), b: device
 *      fp64 [nb], c: device fp64 [1].  Workspace:
 *      flr_fang_krum_strength_workspace(K, nmal) bytes (the sorted rows; 0 for
 *      rejected arguments), 256-byte aligned.
 *      FLR_ERR_ARG: a null G, b, c, lambda64, lambda32 or info; nmal < 1; threshold
 *      not a finite number > 0.  FLR_ERR_KRUM_N: K < 2 nmal + 3, Krum's own
 *      condition.  FLR_ERR_UNSUPPORTED: nb > 1024.  FLR_ERR_WORKSPACE.
 *   5. the rows, two separately rounded fp32 ops per element (no FMA):
 *        out_k = fl(g_k - fl(lambda32 * s_k))
 *      A NaN lambda writes nothing: the rows stay as they were.  A lane owns one
 *      float4 of coordinates, or one coordinate (X or global not 16-byte aligned,
 *      or ldx % 4 != 0): the same bits.
 * lambda_out: optional device fp64 [1]; info_out: optional device int32 [2];
 * stats_out: optional device fp64 [nb + 6]: b_i [nb], c, then the strength call's
 * five; gram_out: optional device fp64 nb x nb, G.  Workspace:
 * flr_fang_krum_workspace(K, P, nmal) bytes (0 for arguments the call rejects),
 * 256-byte aligned: mu, s, G, flr_rows_gram's workspace, the sorted rows, the
 * partial sums.  After the call its first P floats hold mu and the P floats at
 * byte offset (4*P + 255) / 256 * 256 hold s.
 * Bytes moved: 3 * nb * P * 4 read (mean, Gram, statistics) + nmal * P * 4
 * written, as flr_minmax_rows; not timed yet.
 * FLR_ERR_ARG: null X or global, K < 2, nmal < 1, nmal >= K, P < 1, ldx < P,
 * threshold not a finite number > 0.  FLR_ERR_KRUM_N: K < 2 nmal + 3.
 * FLR_ERR_UNSUPPORTED: nb > 1024 (flr_rows_gram's row limit, the one-workgroup
 * solver's too).  FLR_ERR_WORKSPACE: workspace null, too small or not 256-byte
 * aligned.
 *
 * flr_fang_trim_rows, the trimmed-mean / median attack: per coordinate the
 * attackers sit just beyond the benign extreme on the side opposite s, each at a
 * point of its own drawn between two bounds.  One pass reads the benign rows and
 * writes the attackers' rows.  Per coordinate k, fp32, every operation rounded on
 * its own, the benign rows in ascending order:
 *   mu, s: as above.   mn = mx = the first benign value; then per row
 *   mn = x < mn ? x : mn,  mx = x > mx ? x : mx.
 *   s > 0:  mn > 0: (near, far) = (mn, mn / b);  else (mn, mn * b)
 *   s < 0:  mx > 0: (near, far) = (mx, mx * b);  else (mx, mx / b)
 *   attacker i:  out = fl(near + fl(u_ik * fl(far - near)))
 *   s == 0: every attacker gets mu_k.   s NaN (a NaN in a benign row, or in g):
 *   every attacker gets fl(mu_k - g_k), a NaN — in that coordinate and no other.
 *   u_ik = (w >> 8) * 2^-24 in [0, 1), w word 0 of Philox4x32-10 (Salmon, Moraes,
 *   Dror, Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3", SC 2011) with key
 *   (seed & 0xffffffff, seed >> 32) and counter (c & 0xffffffff, c >> 32, i,
 *   draw_stream), c = col0 + k.  Ten rounds; round r = 0..9 on counter (c0, c1,
 *   c2, c3) with key (k0, k1) bumped by (0x9E3779B9, 0xBB67AE85) mod 2^32 before
 *   every round but the first:
 *     p0 = 0xD2511F53 * c0, p1 = 0xCD9E8D57 * c2          (64-bit products)
 *     (c0, c1, c2, c3) <- (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0))
 *   No device RNG library is linked.
 * b: fp32, finite, > 1 (the paper uses 2).  col0 >= 0: the global index of column
 * 0, so a column range of X called with its own col0 (same ldx) gives that range
 * of the whole-matrix call, bit for bit.  draw_stream: the round index.  Any K
 * with 1 <= nmal < K; no workspace.  A lane owns one float4 of coordinates, or one
 * coordinate (as above: the same bits).
 * Bytes moved: nb * P * 4 + P * 4 read, nmal * P * 4 written.
 * FLR_ERR_ARG: null X or global, K < 2, nmal < 1, nmal >= K, P < 1, ldx < P, b not
 * a finite number > 1, col0 < 0 or col0 + P past 2^63 - 1. */
#define FLR_FANG_THRESHOLD 1e-5 /* the paper's */
size_t flr_fang_krum_strength_workspace(int64_t K, int64_t nmal);
int flr_fang_krum_strength(const double* G, const double* b, const double* c, int64_t K,
                           int64_t nmal, double threshold, double* lambda64, float* lambda32,
                           int32_t* info, double* stats_out, void* workspace,
                           size_t workspace_bytes, void* stream);
size_t flr_fang_krum_workspace(int64_t K, int64_t P, int64_t nmal);
int flr_fang_krum_rows(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal,
                       const float* global, double threshold, double* lambda_out,
                       int32_t* info_out, double* stats_out, double* gram_out,
                       void* workspace, size_t workspace_bytes, void* stream);
int flr_fang_trim_rows(float* X, int64_t K, int64_t P, int64_t ldx, int64_t nmal,
                       const float* global, float b, uint64_t seed, uint32_t draw_stream,
                       int64_t col0, void* stream);

/* ---- centered clipping (Karimireddy, He, Jaggi, ICML 2021) ---------------
 * "Learning from History for Byzantine Robust Optimization": from the previous
 * global model v0, iters times
 *   v <- v + (1/K) * sum_i (x_i - v) * min(1, tau / ||x_i - v||)
 * so one call moves the aggregate by at most iters * tau however the attackers
 * collude.  No reference counterpart.  The whole loop is enqueued on the stream,
 * no host synchronisation.  Iteration l = 0 .. iters-1, v_0 = v0:
 *   1. distances (flr_row_norms, type 0, center v_l): d_i = ||x_i - v_l||, fp32
 *      differences, squares summed in fp64 in a fixed order, fp64 square root.
 *   2. scales, fp32 throughout: d32_i = (float)d_i (round to nearest);
 *        t = tau when tau > 0; when tau == 0 (adaptive mode) t = the lower median
 *            of the K values d32, sort(d32)[(K-1)/2] with NaN sorted last (numpy's
 *            order): at most half the rows are clipped;
 *        s_i = 0 if d32_i is NaN;  else t / d32_i if d32_i > t (one correctly
 *              rounded division; +inf gives 0);  else 1.
 *      A median t of NaN compares false with everything (every non-NaN row keeps
 *      s_i = 1); a median t of 0 gives every row at a positive distance s_i = 0.
 *   3. step, per coordinate, the rows in ascending order, every operation a
 *      separately rounded fp32 op (no FMA):
 *        acc = +0.f
 *        for i in 0..K-1:  if s_i != 0:  acc = acc + (x_i - v) * s_i
 *        v' = v + acc / (float)K
 *      A row with s_i == 0 is skipped, not multiplied: a client holding a NaN or
 *      an inf (distance NaN or +inf) leaves the aggregate finite, as Krum ranks
 *      such a client last.  The divisor stays K.
 * so a torch CPU loop over the rows, given the distances, gives the same bits.
 * out: device fp32 [P], v_iters; must not be v0 (the iterates alternate between
 * out and a P-vector of the workspace; v0 is only read).  Optional device
 * outputs (NULL: not written): norms_out fp64 [iters][K], the d_i; scales_out
 * fp32 [iters][K], the s_i; tau_out fp32 [iters], the t used.  Columns [P, ldx)
 * of X are never touched.  Bytes moved: 2 * iters * K * P * 4 (the distance pass
 * and the step each read X once).
 * FLR_ERR_ARG: null X, v0 or out; K < 1; P < 1; ldx < P; iters < 1; tau < 0 or
 * NaN; out == v0.  FLR_ERR_WORKSPACE: workspace null, smaller than
 * flr_centered_clip_workspace(K, P) (0 for K < 1 or P < 1) or not 256-byte
 * aligned.  FLR_ERR_UNSUPPORTED: K > 4096 (the scales kernel is one workgroup;
 * flr_weighted_rows' row limit).  Nothing is written on an error. */
size_t flr_centered_clip_workspace(int64_t K, int64_t P);
int flr_centered_clip(const float* X, int64_t K, int64_t P, int64_t ldx,
                      const float* v0, float tau, int64_t iters, float* out,
                      double* norms_out, float* scales_out, float* tau_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- divide-and-conquer, DnC (Shejwalkar, Houmansadr, NDSS 2021) ---------
 * "Manipulating the Byzantine", Algorithm 2: the spectral defense of the paper
 * that Min-Max and Min-Sum (flr_minmax_rows) come from.  No reference
 * counterpart.  The clients are projected on the top right singular vector of
 * the centered, column-subsampled client matrix and the nremove largest squared
 * projections are dropped: it catches attackers that collude along one
 * direction inside the benign spread, which distances and per-coordinate order
 * do not.  All niters iterations are enqueued on the stream, no host
 * synchronisation.  Iteration it = 0 .. niters-1:
 *   1. columns: b distinct columns of [0, P), ascending, one per stratum:
 *        lo_j = floor(j*P/b), hi_j = floor((j+1)*P/b),
 *        col_j = lo_j + h % (hi_j - lo_j),
 *        h = mix(seed + 0x9E3779B97F4A7C15 * (it*b + j + 1))   (mod 2^64),
 *        mix(z): z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27;
 *                z *= 0x94D049BB133111EB; z ^= z>>31   (splitmix64's finaliser),
 *      generated on the device.  cols (optional, device int64 [niters][b])
 *      replaces them: each value is clamped into [0, P-1] on the device; they
 *      need not be sorted or distinct.
 *   2. bad rows: a row with a NaN or +-inf among its b sampled values is bad in
 *      this iteration: left out of the mean, its centered row all zeros, its
 *      score +inf, never kept.
 *   3. center, per sampled column, every operation a separately rounded fp32 op
 *      (no FMA), as flr_collude_rows' mean:
 *        s = +0.f;  for the good rows i ascending: s = s + x_ij
 *        mu_j = s / (float)ngood;   c_ij = x_ij - mu_j
 *   4. Gram: G_ik = sum_j (double)c_ij * (double)c_kj, the products exact in
 *      fp64, summed in a fixed order (chunks of columns chosen from K and b,
 *      ascending inside a chunk, the chunks' sums added in order).  The
 *      singular vector is never formed: for w = G u the projection of row i on
 *      it is w_i / sqrt(u.w).
 *   5. power iteration, fp64 (the sums in a fixed order, the same bits from run
 *      to run):  a = the index of the largest G_aa, the lowest on ties;
 *        u = G[:,a] / ||G[:,a]||    (the all-ones vector is in G's null space:
 *                                    C is column-centered)
 *        power_iters times:  w = G u;  u = w / ||w||
 *        w = G u;  lam = u.w;  score_i = w_i * w_i / lam
 *      Every good row scores 0 when G_aa == 0, a ||w|| is 0 or lam <= 0 (one
 *      client, identical rows).
 *   6. keep: the K scores ranked ascending, equal scores to the lower index, the
 *      bad rows last in index order; the iteration keeps the good rows with
 *      rank < K - nremove.
 * keep: device int32 [K], 1 for the rows every iteration kept, else 0; when no
 * row is in that intersection keep is iteration 0's set and bit 0 of flags_out
 * is set (with every row bad that set is empty too: count 0).  count: device
 * int32 [1], the number of ones.  Optional device outputs (NULL: not written):
 * scores_out fp64 [niters][K]; cols_out int64 [niters][b], the columns used;
 * flags_out int32 [1].  X, columns [P, ldx) included, is only read.
 * Workspace: flr_dnc_workspace(K, b) bytes (0 for arguments the call rejects),
 * 256-byte aligned: the compact K x b matrix, G and its partial sums, the
 * flags.  Bytes moved per iteration: K * b * 4 gathered, the compact matrix
 * read about 2 + K/8 times from L2.
 * FLR_ERR_ARG: null X, keep or count; K < 1; b < 1; b > P; ldx < P; niters < 1;
 * power_iters < 1; nremove outside [0, K-1].  FLR_ERR_UNSUPPORTED: K > 1024
 * (the spectral kernel is one workgroup, a lane per client), b > 65536,
 * niters > 16, power_iters > 1024.  FLR_ERR_WORKSPACE: workspace null, too small
 * or not 256-byte aligned.  Nothing is written on an error. */
size_t flr_dnc_workspace(int64_t K, int64_t b);
int flr_dnc_select(const float* X, int64_t K, int64_t P, int64_t ldx, int64_t b,
                   int64_t niters, int64_t nremove, int64_t power_iters,
                   uint64_t seed, const int64_t* cols, int32_t* keep,
                   int32_t* count, double* scores_out, int64_t* cols_out,
                   int32_t* flags_out, void* workspace, size_t workspace_bytes,
                   void* stream);
/* The mean of the rows with keep[i] != 0 (keep: device int32 [K], e.g.
 * flr_dnc_select's), counted on the device — no host round trip between the
 * selection and the mean:
 *   acc = +0.f;  for the kept rows i ascending: acc = acc + x_i;
 *   out = acc / (float)count           (fp32, every op separately rounded)
 * bit-identical to flr_rows_mean over the ascending kept list with divisor =
 * count.  No row kept: 0 / 0, NaN in every coordinate.  Only the kept rows are
 * read (a NaN in a skipped row leaves out finite); count * P * 4 bytes.
 * FLR_ERR_ARG: null X, keep or out; K < 1; P < 0; ldx < P.
 * FLR_ERR_UNSUPPORTED: K > 4096.  Nothing is written on an error. */
int flr_rows_mean_keep(const float* X, int64_t K, int64_t P, int64_t ldx,
                       const int32_t* keep, float* out, void* stream);

/* ---- FoolsGold (Fung, Yoon, Beschastnikh, RAID 2020) ----------------------
 * "The Limitations of Federated Learning in Sybil Settings", Algorithm 1: the
 * sybil defense.  No reference counterpart.  Clients whose (accumulated) updates
 * point the same way lose their weight: it needs no attacker count and no server
 * data, and catches the attackers that act in concert (the colluding attacks'
 * identical rows, a common backdoor).  Four calls: history, Gram matrix,
 * weights, combination.  Each enqueues all its work on the stream with no host
 * synchronisation, never touches columns [P, ld) and writes nothing on an error.
 *
 * flr_rows_accumulate, the history update, in place, per element two separately
 * rounded fp32 operations (no FMA):
 *   H_ij = fl(H_ij + fl(X_ij - center_j))
 * H, X: device fp32 K x P (row strides ldh, ldx); center: device fp32 [P].
 * Bytes moved: 3 * K * P * 4 (H read and written, X read).
 * FLR_ERR_ARG: null H, X or center; K < 1; P < 1; ldh < P; ldx < P; H == X.
 * FLR_ERR_UNSUPPORTED: K > 65535. */
int flr_rows_accumulate(float* H, int64_t ldh, const float* X, int64_t ldx,
                        const float* center, int64_t K, int64_t P, void* stream);
/* flr_rows_gram, the K x K Gram matrix of the rows over all P coordinates:
 *   G_ij = sum_p (double)a_ip * (double)a_jp
 *   a_ip = A_ip when center is NULL, else fl(A_ip - center_p) (one fp32
 *          subtraction)
 * G: device fp64 [K][K], written whole and symmetric: G_ij and G_ji are the same
 * bits (one sum, stored twice).  The products run on v_mfma_f64_16x16x4_f64 and
 * are exact (an fp32 converts to fp64 exactly; the product of two has 48
 * significant bits); the sums are fp64.  The order of the sums is a function of
 * (K, P) alone, the same on the aligned and the unaligned path, so a rerun gives
 * the same bits: the columns are cut into flr_rows_gram_splits(K, P) chunks of
 *   c = max(256, 64 * ceil(ceil(P / max(1, floor(2048 / T))) / 64)) columns,
 *   T = n (n + 1) / 2, n = ceil(K / 64)     (T <= 136 for K <= 1024)
 * one workgroup per 64 x 64 block on or above the diagonal and chunk; inside a
 * chunk the columns go by in groups of 16, MFMA s (0..3) of a group summing its
 * columns s, s + 4, s + 8, s + 12; a second kernel adds the chunks' partial
 * entries in chunk order (no second kernel for one chunk).  Blocks below the
 * diagonal are not computed.  Rows past K and columns past P enter as zeros
 * through guarded loads; nothing is read past row K - 1 or column P - 1.  Any
 * lda >= P; rows need no alignment beyond 4 bytes (A and center 16-byte aligned
 * and lda % 4 == 0: 16-byte loads, the same bits).  A NaN or inf in row i makes
 * G_ii NaN or inf (the weights' bad-row test).
 * Workspace: flr_rows_gram_workspace(K, P) bytes (splits * K * K * 8, rounded up
 * to 256; 0 for one chunk and for arguments the call rejects), 256-byte aligned.
 * Bytes moved: every 64-row block is read by the n block pairs it is part of,
 * n * K * P * 4 in all (the pairs of a chunk are adjacent workgroups, so the
 * repeats mostly come from L2), plus 2 * splits * K * K * 8 for the partial
 * matrices.
 * FLR_ERR_ARG: null A or G; K < 1; P < 1; lda < P.  FLR_ERR_UNSUPPORTED: K >
 * 1024.  FLR_ERR_WORKSPACE (more than one chunk): workspace null, too small or
 * not 256-byte aligned. */
size_t flr_rows_gram_workspace(int64_t K, int64_t P);
int64_t flr_rows_gram_splits(int64_t K, int64_t P); /* 0 for rejected arguments */
int flr_rows_gram(const float* A, int64_t K, int64_t P, int64_t lda,
                  const float* center /* may be NULL */, double* G,
                  void* workspace, size_t workspace_bytes, void* stream);
/* flr_foolsgold_weights: the clients' weights from the Gram matrix of their
 * rows.  One workgroup, a lane per client; all arithmetic fp64, in this order:
 *   row i is bad when G_ii is not finite: alpha_i = 0, it takes no part in
 *     anyone's maximum; any bad row sets bit 1 of flags.
 *   n_i = sqrt(G_ii)
 *   cs_ij = G_ij / (n_i * n_j) for i != j when both rows are good and n_i > 0
 *     and n_j > 0, else 0; cs_ii = 0 (the original subtracts the identity).  G
 *     is taken as symmetric: the kernel reads G_ji for cs_ij.
 *   v_i = max_j cs_ij  (>= 0 because of the diagonal): maxcos_out.
 *   pardoning: pc_ij = cs_ij * v_i / v_j when v_i < v_j (multiply, then divide),
 *     else cs_ij.
 *   w_i = min(1, max(0, 1 - max_j pc_ij))
 *   top = max_i w_i over the good rows.  top == 0 or every row bad: every
 *     alpha_i = 0, every beta_i = 0, bit 0 of flags (the paper's "no update").
 *   else w_i = min(w_i / top, 0.99);
 *     alpha_i = min(1, max(0, kappa * (log(w_i / (1 - w_i)) + 0.5)))
 *     (w_i = 0: the logarithm is -inf, alpha_i = 0).
 *   S = sum_i alpha_i, ascending in i; beta_i = (float)(alpha_i / S); S == 0:
 *     every beta_i = 0 and bit 0 of flags.
 *   K = 1: alpha = beta = 1 for a good row.
 * A maximum ignores a NaN operand.  min(w, 0.99) replaces the original code's
 * wv[wv == 1] = .99: it is continuous in w, and at the paper's kappa = 1 it
 * gives the same weights (every w in [0.99, 1) has kappa * (logit + 0.5) > 1
 * already, so both forms clip to alpha = 1).
 * alpha: device fp64 [K]; beta: device fp32 [K]; optional (NULL: not written)
 * maxcos_out fp64 [K], flags_out int32 [1].  Bytes: G read twice (L2).
 * FLR_ERR_ARG: null G, alpha or beta; K < 1; kappa not a finite number > 0.
 * FLR_ERR_UNSUPPORTED: K > 1024. */
int flr_foolsgold_weights(const double* G, int64_t K, double kappa, double* alpha,
                          float* beta, double* maxcos_out /* optional */,
                          int32_t* flags_out /* optional */, void* stream);
/* flr_rows_combine_from: per coordinate, the rows in ascending order, every
 * operation a separately rounded fp32 op (no FMA), as flr_centered_clip's step:
 *   acc = +0.f
 *   for i in 0..K-1:  if beta_i != 0:  acc = acc + (x_i - c) * beta_i
 *   out = c + acc
 * beta: device fp32 [K] (flr_foolsgold_weights').  A row with beta_i == 0 is not
 * read: a NaN in a rejected row leaves out finite.  All beta zero: out == center
 * bit for bit.  Bytes moved: (rows with beta != 0) * P * 4 read, P * 4 written.
 * FLR_ERR_ARG: null X, center, beta or out; K < 1; P < 1; ldx < P; out ==
 * center.  FLR_ERR_UNSUPPORTED: K > 4096. */
int flr_rows_combine_from(const float* X, int64_t K, int64_t P, int64_t ldx,
                          const float* center, const float* beta /* device [K] */,
                          float* out, void* stream);

/* ---- FLAME (Nguyen et al., USENIX Security 2022) ---------------------------
 * "FLAME: Taming Backdoors in Federated Learning", Algorithm 1: the backdoor
 * defense.  No reference counterpart.  The clients are clustered by the cosine
 * distances of their updates, the majority cluster is admitted, the admitted
 * updates are clipped to the median update norm and averaged, and Gaussian noise
 * scaled by that median is added.  It needs no attacker count and no server
 * data.  Four calls: flr_rows_gram (above), flr_flame_select, flr_rows_combine_from
 * (above) and flr_add_gaussian, each enqueued on the stream with no host
 * synchronisation; nothing is written on an error.
 *
 * flr_flame_select: one launch of one workgroup, a lane per client.  With G the
 * Gram matrix of the updates u_i = x_i - g (flr_rows_gram with center g; with no
 * center the paper's Algorithm 1 read literally, the cosines of the models), all
 * arithmetic fp64, every operation rounded on its own, only + - * / sqrt:
 *   1. distances.  n_i = sqrt(G_ii).  Row i is bad when G_ii is not finite: it has
 *      no edges, is never admitted, and sets bit 1 of flags.  For i != j, both
 *      good:  d_ij = 1 when n_i == 0 or n_j == 0, else
 *        d_ij = 1 - G_ij / (n_i * n_j)     (the product, the quotient, the
 *                                           subtraction; not clamped)
 *      A NaN d_ij is no edge.  G is taken as symmetric (flr_rows_gram's is, bit
 *      for bit): the kernel reads G_ji for d_ij.
 *   2. clustering.  The paper calls HDBSCAN with min_cluster_size = m = K/2 + 1
 *      (integer division), min_samples = 1, allow_single_cluster = True on these
 *      distances.  Two facts give that call a closed form:
 *        - the core distance of a point (min_samples = 1: the distance to its
 *          nearest neighbour) is at most its distance to anyone, so the mutual
 *          reachability distance max(core_i, core_j, d_ij) is d_ij itself;
 *        - with 2 m > K two clusters of m points cannot coexist, so the
 *          condensed tree never splits: the one selected cluster is the first
 *          single-linkage component that reaches m points.
 *      So: t* = the smallest t for which the graph on the good rows with the
 *      edges {d_ij <= t} has a connected component of at least m rows; that
 *      component is admitted (it is unique: two would hold more than K rows),
 *      every other row is rejected.  Edges of equal weight enter together, so no
 *      tie-breaking order exists that could change the result.  The kernel runs
 *      Prim's minimum spanning tree over the implicit distance matrix (lane j
 *      keeps its key, each step reads one row of G coalesced and ends in a
 *      workgroup arg-min), sorts the K - 1 tree edges in LDS and merges them level
 *      by level until a component holds m rows: the components of any minimum
 *      spanning tree cut at t are those of the threshold graph, so ties in
 *      Prim's choice cannot change the answer either.
 *      Because the cluster is cut the moment it reaches m, the rule typically
 *      admits m or m + 1 clients, about half: that is the published rule, and m
 *      is the knob.
 *   3. fewer than m good rows, or no component of m rows (NaN distances): no
 *      cluster.  keep is all 0, every beta 0, sigma 0, t* = +inf, L = 0, bit 0 of
 *      flags; flr_rows_combine_from then returns the center bit for bit.
 *      m == 1 (only K == 1 allows it): the good row is admitted, t* = 0.
 *   4. clipping bound.  e_i = norms[i] when norms is given (the caller's update
 *      norms when G was taken without a center: flr_row_norms about g), else
 *      n_i.  S = the lower median of the K values e, sort(e)[(K-1)/2] with NaN
 *      sorted last (flr_centered_clip's convention), over all clients, rejected
 *      ones included, as in the paper.  L = the admitted count.
 *        gamma_i = S / e_i when e_i > S, else 1
 *        beta_i  = (float)(gamma_i / L) for an admitted row, exactly 0.f for a
 *                  rejected one
 *        sigma   = (float)(lambda * S); 0.f with no cluster
 * Given the same G bits a numpy restatement of steps 1-4 therefore gives the
 * same keep, t*, S, L, beta, sigma and flags bit for bit (sqrt and the four
 * operations are correctly rounded on the device; the library is built with
 * -ffp-contract=off): tests/flame_ref.py is that restatement.
 * G: device fp64 [K][K]; norms: optional device fp64 [K]; keep: device int32
 * [K], 1 admitted, 0 rejected; beta: device fp32 [K]; sigma: device fp32 [1];
 * optional (NULL: not written) stats fp64 [3]: S, t*, L; flags int32 [1].
 * Bytes: G read once (one row per step; 8 MB at K = 1024, from L2).  About K
 * dependent steps: latency-bound.
 * FLR_ERR_ARG: null G, keep, beta or sigma; K < 1; m > K or 2 m <= K; lambda
 * negative, NaN or infinite.  FLR_ERR_UNSUPPORTED: K > 1024 (flr_rows_gram's
 * limit; one lane per client). */
int flr_flame_select(const double* G, const double* norms /* optional */, int64_t K, int64_t m,
                     double lambda, int32_t* keep, float* beta, float* sigma /* device [1] */,
                     double* stats /* optional: S, t*, L */, int32_t* flags /* optional */,
                     void* stream);
/* flr_add_gaussian: v_k <- fl(v_k + fl(sigma * z_k)) in place, k = 0 .. P-1, two
 * separately rounded fp32 operations; z standard normal.  sigma: device fp32 [1]
 * (flr_flame_select's); sigma == 0 leaves every bit of v as it is (-0.f
 * included).  The four consecutive global coordinate indices 4c .. 4c+3,
 * c = (col0 + k) >> 2, share one Philox4x32-10 block (the round is written out
 * at flr_fang_trim_rows) with key (seed & 0xffffffff, seed >> 32) and counter
 * (c & 0xffffffff, c >> 32, 0, draw_stream).  With its words w0..w3, fp32:
 *   u1 = ((w0 >> 8) + 1) * 2^-24  in (0, 1];   u2 = (w1 >> 8) * 2^-24  in [0, 1)
 *   r  = sqrtf(fl(-2 * logf(u1)));  a = fl(6.2831853071795864769f * u2)
 *   z0 = fl(r * cosf(a));  z1 = fl(r * sinf(a))
 * z2 and z3 come from (w2, w3) in the same way; index 4c + j takes z_j.  logf,
 * sinf and cosf are the accurate library functions, not the fast intrinsics
 * (within 1e-5 absolute of the fp64 evaluation; |z| <= sqrt(48 ln 2) < 5.78).
 * col0 >= 0: the global index of v[0], so a column range called with its own
 * col0 gives that range of the whole call bit for bit.  A lane owns one Philox
 * block: the lanes at the two ends compute a whole block and use the part of it
 * inside [0, P).  The block's four floats move in one 16-byte access when their
 * address is 16-byte aligned ((address of v) / 4 - col0 a multiple of 4), else
 * in four 4-byte accesses: the same bits.  Bytes moved: 8 * P.
 * FLR_ERR_ARG: null v or sigma; P < 0; col0 < 0 or col0 + P past 2^63 - 1.
 * FLR_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups of 256 blocks (P beyond
 * 2^41).  P == 0: FLR_OK, nothing enqueued. */
int flr_add_gaussian(float* v, int64_t P, const float* sigma /* device [1] */, uint64_t seed,
                     uint32_t draw_stream, int64_t col0, void* stream);

/* ---- the robust learning rate, RLR (Ozdayi, Kantarcioglu, Gel, AAAI 2021) ----
 * "Defending against Backdoors in Federated Learning with Robust Learning Rate":
 * per coordinate the clients vote with the sign of their update against the
 * round's global model g, and where fewer than theta net votes agree the
 * server's learning rate for that coordinate is negated, so the aggregate moves
 * away from an unopposed minority.  The rule wraps any base aggregate agg.  No
 * reference counterpart.  Every entry enqueues on the stream and never
 * synchronises with the host; columns [P, ldx) of X are never touched.
 *
 * flr_sign_vote: for every coordinate p
 *     votes[p] = #{k : X[k][p] > g[p]} - #{k : X[k][p] < g[p]}
 *   Comparisons only, no arithmetic on the values (no rounding or denormal
 *   question): a NaN on either side votes 0, -0 against +0 votes 0, +-inf votes
 *   by its sign (against an equal inf: 0).  votes: device int32 [P], an exact
 *   integer in [-K, K], the same with 16-byte and 4-byte loads.  The K rows are
 *   streamed with 16 loads in flight per lane.  Bytes moved: K * P * 4 + 8 * P.
 *
 * flr_rlr_apply: per coordinate, every operation a separately rounded fp32 op
 * (no FMA):
 *     d    = agg - g
 *     pass = |votes| >= theta
 *     out  = agg            when pass and eta == 1   (the base aggregate's bits)
 *          = g + eta * d    when pass and eta != 1
 *          = g - eta * d    when not pass
 *   so a CPU loop gives the same bits.  agg, g: device fp32 [P]; votes: device
 *   int32 [P]; out: device fp32 [P], may be agg (in place), must not be g.
 *   flipped: optional (NULL: not written) device int64 [1], the number of
 *   coordinates with pass false: the call zeroes it on the stream, then each
 *   workgroup adds its count with one atomicAdd.  Bytes moved: 16 * P.
 *
 * flr_rlr_fedavg: the fused default, one pass over X for the vote and the FedAvg
 * sum.  The accumulator is flr_fedavg's: weights (float)n_i, fl(n_i * x) added
 * in client order from +0, one division by (float)sum_i n_i.  out, votes_out
 * (optional, device int32 [P]) and flipped (optional) equal bit for bit what
 * flr_fedavg, then flr_sign_vote, then flr_rlr_apply produce.  num_examples:
 * device int64 [K].  One lane owns one float4 of coordinates (or one coordinate:
 * a pointer not 16-B aligned or ldx % 4 != 0) with W float accumulators and W
 * int counters; the rows are streamed in row order.  Bytes moved: K * P * 4 +
 * 8 * P (+ 4 * P with votes_out).
 *
 * FLR_ERR_ARG: a null required pointer; K < 1; P < 0; ldx < P; theta < 0 or
 * theta > K (flr_rlr_apply, which takes no K: theta < 0); eta not finite or
 * <= 0; out == g.  FLR_ERR_UNSUPPORTED: K > 4096 (flr_fedavg's limit, kept for
 * flr_sign_vote too: the composition and the fused call accept the same shapes).
 * P == 0: FLR_OK, flipped = 0.  Nothing is written on an error. */
int flr_sign_vote(const float* X, int64_t K, int64_t P, int64_t ldx, const float* g,
                  int32_t* votes, void* stream);
int flr_rlr_apply(const float* agg, const float* g, const int32_t* votes, int64_t P,
                  int64_t theta, float eta, float* out, int64_t* flipped /* optional */,
                  void* stream);
int flr_rlr_fedavg(const float* X, int64_t K, int64_t P, int64_t ldx,
                   const int64_t* num_examples, const float* g, int64_t theta, float eta,
                   float* out, int32_t* votes_out /* optional */,
                   int64_t* flipped /* optional */, void* stream);

/* ---- SparseFed (Panda et al., AISTATS 2022) and the magnitude top-k ---------
 * "SparseFed: Mitigating Model Poisoning Attacks in Federated Learning with
 * Sparsification", Algorithm 1: the clients' updates are clipped to a norm L and
 * averaged, the average is added to a server-side error memory W, only the k
 * largest-magnitude coordinates of W are applied to the model, and the rest stay
 * in W for later rounds.  No reference counterpart.  With g the round's global
 * model, x_i row i of X, rho the momentum, W and U (the momentum's memory) device
 * fp32 [P] state of the caller, +0 at first use.  Every fp32 operation is rounded
 * on its own (no FMA).  Calls: flr_row_norms (e_i = ||x_i - g||, fp64),
 * flr_sparsefed_weights, flr_sparsefed_accumulate, flr_topk_abs_select,
 * flr_sparsefed_apply, each enqueued on the stream: nothing is allocated or
 * copied to the host inside them, so they can be captured into a graph; nothing
 * is written on an error.  tests/sparsefed_ref.py restates the arithmetic.
 *
 * flr_sparsefed_weights: one workgroup, fp64, only + - * / and comparisons.
 *   Row i is bad when e_i (norms[i]) is not finite: beta_i = 0.f exactly (the
 *     later passes do not read it: flr_rows_combine_from's convention) and bit 1
 *     of flags.
 *   n = the number of good rows.  n == 0: every beta 0, L = 0, bit 0 of flags.
 *   L = clip_norm when it is > 0, else (clip_norm == 0) the lower median of the
 *     good rows' e, sorted[(n - 1) / 2].  The adaptive default is this library's
 *     choice, as FLAME's bound is; the paper's L is a tuned constant.
 *   gamma_i = L / e_i when e_i > L, else 1;  beta_i = (float)(gamma_i / n).
 *   norms: device fp64 [K]; beta: device fp32 [K]; optional (NULL: not written)
 *   stats fp64 [3]: L, n, the number of rows with e_i > L; flags int32 [1].
 *   FLR_ERR_ARG: null norms or beta; K < 1; clip_norm negative, NaN or infinite.
 *   FLR_ERR_UNSUPPORTED: K > 4096.
 *
 * flr_sparsefed_accumulate: the K x P pass.  Per coordinate p:
 *     a = +0;  for i in 0..K-1:  if beta_i != 0:  a = a + (x_i[p] - g[p]) * beta_i
 *   (flr_rows_combine_from's accumulator without the final + c; a row with beta_i
 *   == 0 is not read)
 *     rho != 0:  u = rho * U[p] + a   (the product, then the sum);  U[p] = u
 *     rho == 0:  u = a; U is not touched and may be NULL
 *     w = W[p] + u
 *     w not finite:  W[p] = +0, with rho != 0 also U[p] = +0, and the coordinate
 *                    counts into dropped;  else W[p] = w
 *   and the key (below) of the stored W[p] is counted into hist, the level-1
 *   histogram flr_topk_abs_select takes.  hist: optional device uint32 [2048];
 *   dropped: optional device int64 [1]; the call zeroes both on the stream first.
 *   Each workgroup counts into a private LDS histogram and flushes it with one
 *   integer atomicAdd per non-empty bin; dropped is one atomicAdd per workgroup:
 *   integer sums, the same from run to run.  One lane owns one float4 of
 *   coordinates, or one coordinate when a pointer is not 16-byte aligned or ldx % 4
 *   != 0: the same bits.  Columns [P, ldx) are never touched; X, g and beta are
 *   only read.  Bytes moved: (rows with beta != 0) * P * 4 + 12 * P (+ 8 * P with
 *   the momentum).
 *   FLR_ERR_ARG: null X, g, beta or W; K < 1; P < 0; ldx < P; rho outside [0, 1)
 *   or NaN; rho != 0 with a null U; W, U and g not distinct.
 *   FLR_ERR_UNSUPPORTED: K > 4096; P >= 2^32 (the counts are 32-bit).
 *   P == 0: FLR_OK, nothing enqueued.
 *
 * flr_topk_abs_select: the exact, deterministic magnitude top-k of any fp32
 * vector v [P], 1 <= k <= P.
 *     key(v) = bits(v) & 0x7fffffff when that is below 0x7f800000, else 0
 *   a NaN or an inf ranks with zero and sets bit 0 of the flags.  A radix select
 *   on three digits of the 31-bit key, d1 = key >> 20 (2048 bins), d2 = (key >> 9)
 *   & 0x7ff (2048 bins), d3 = key & 0x1ff (512 bins): per level a histogram pass
 *   over v that counts the keys matching the digits found so far, and a
 *   one-workgroup scan from the top bin down to the bin where the running count
 *   reaches the remaining k.  hist1: optional device uint32 [2048], the level-1
 *   histogram of v's keys (flr_sparsefed_accumulate's): level 1's pass over v is
 *   then skipped; the result is the same.  It must be the histogram of this v as
 *   it stands: with another one the scans may find no bin, and sel is then left
 *   unwritten or names a threshold that is not v's.  Then a count pass gives each chunk's
 *   number of keys == T (a chunk: 1024 adjacent coordinates; the chunk map is a
 *   function of P alone) and a one-workgroup exclusive scan over the chunks leaves
 *   the ties' prefix in the workspace, for flr_topk_abs_mask / flr_sparsefed_apply.
 *   sel: device uint32 [4]:  T, the key of the k-th largest;  n_gt, the number
 *   of keys > T;  r = k - n_gt, 1 <= r <= n_eq (the number of keys == T);  the
 *   flags.  Coordinate p is selected when key > T, or key == T and fewer than r
 *   coordinates q < p have key == T: the lowest indices win, as in a stable
 *   descending sort of the keys.  k == P selects everything.  No kernel waits on
 *   another workgroup: every dependency is a kernel boundary on the stream.
 *   workspace: flr_topk_abs_workspace(P) bytes, 256-byte aligned (0 for a
 *   rejected P): the histograms and the per-chunk tie counts; a later mask or
 *   apply call reads it, so it must stay untouched between the calls.  Bytes
 *   moved: 16 * P (12 * P with hist1), from the Infinity Cache when v fits.
 *   FLR_ERR_ARG: null v or sel; P < 0; k outside [1, P].  FLR_ERR_UNSUPPORTED:
 *   P >= 2^32.  FLR_ERR_WORKSPACE.  P == 0: FLR_OK, nothing enqueued.
 *
 * flr_topk_abs_mask: mask[p] = 1 for a selected coordinate, else 0, from sel and
 * the workspace of flr_topk_abs_select on the same v.  mask: device uint8 [P].
 * The in-chunk tie rank is a wave ballot prefix, then the waves' counts through
 * LDS.  Bytes moved: 5 * P.
 *
 * flr_sparsefed_apply: with sel and the workspace of flr_topk_abs_select on W,
 *     selected:      out[p] = g[p] + W[p];  W[p] = +0;  U[p] = +0 when U is given
 *                    (FetchSGD's momentum masking)
 *     not selected:  out[p] = g[p], the same bits
 *   out must not be g or W; U optional; mask: optional device uint8 [P], as
 *   flr_topk_abs_mask's.  Bytes moved: 12 * P (+ P with mask) and 4 * k per state
 *   vector.
 *   FLR_ERR_ARG (both): a null required pointer; P < 0; out == g, out == W, or g,
 *   W, U not distinct.  FLR_ERR_UNSUPPORTED: P >= 2^32.  FLR_ERR_WORKSPACE.
 *   P == 0: FLR_OK, nothing enqueued. */
int flr_sparsefed_weights(const double* norms, int64_t K, double clip_norm /* 0: the median */,
                          float* beta, double* stats /* optional: L, n, clipped */,
                          int32_t* flags /* optional */, void* stream);
int flr_sparsefed_accumulate(const float* X, int64_t K, int64_t P, int64_t ldx, const float* g,
                             const float* beta /* device [K] */, float rho, float* W,
                             float* U /* NULL allowed when rho == 0 */,
                             uint32_t* hist /* optional, device [2048] */,
                             int64_t* dropped /* optional */, void* stream);
size_t flr_topk_abs_workspace(int64_t P);
int flr_topk_abs_select(const float* v, int64_t P, int64_t k,
                        const uint32_t* hist1 /* optional, device [2048] */,
                        uint32_t* sel /* device [4] */, void* workspace, size_t workspace_bytes,
                        void* stream);
int flr_topk_abs_mask(const float* v, int64_t P, const uint32_t* sel, const void* workspace,
                      size_t workspace_bytes, uint8_t* mask, void* stream);
int flr_sparsefed_apply(const float* g, float* W, float* U /* optional */, int64_t P,
                        const uint32_t* sel, const void* workspace, size_t workspace_bytes,
                        float* out, uint8_t* mask /* optional */, void* stream);

/* ---- a6 + a7: fused gradient clip + SGD-momentum step -----------------
 * Replaces, for every client row at once, clip_grad_norm_(params, max_norm)
 * + torch.optim.SGD(lr, momentum, weight_decay).step()
 * (experiments/run_experiments.py:206-211, 234-235; fl_client.py:123-141):
 *   coef_k = min(1, max_norm / (||G_k|| + 1e-6))   (skipped if max_norm <= 0)
 *   g = coef_k*G_k + wd*X_k;  M_k = first ? g : momentum*M_k + g;  X_k -= lr*M_k
 * X, G, M: device fp32 K×P (row stride ld), updated in place.  norms_out:
 * optional device fp32 [K] (pre-clip gradient norms).
 */
size_t flr_clip_sgd_workspace(int64_t K);
int flr_clip_sgd_step(float* X, const float* G, float* M, int64_t K, int64_t P,
                      int64_t ld, float lr, float momentum, float weight_decay,
                      float max_norm, int first_step, float* norms_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Same step on the parameter-major training layout: block j holds block_numel[j]
 * elements per client at client stride block_client_stride[j] (NULL: the
 * blocks are whole parameters, stride = numel); x/g/m_blocks are host arrays
 * of nblocks device pointers (nblocks <= 640, run as launches of <= 80 blocks).  Client k's element e of block j
 * is at ptr_j + k*stride_j + e.  Elements not covered by any block (dead
 * kernel taps, whose gradient is identically zero) are neither read nor
 * updated; with weight_decay == 0 that is exactly the reference's update.
 * first_step is a flag word here: bit 0 = first step (as above), bit 1 = the
 * optimizer's last step (the momentum buffer is not written back: the
 * reference re-creates the optimizer per client per round,
 * run_experiments.py:206-211, so a last step's buffer is never read). */
int flr_clip_sgd_step_blocked(float* const* x_blocks, const float* const* g_blocks,
                              float* const* m_blocks, const int64_t* block_numel,
                              const int64_t* block_client_stride,
                              int64_t nblocks, int64_t K, float lr, float momentum,
                              float weight_decay, float max_norm, int first_step,
                              float* norms_out, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The same step; on the LAST step (first_step bit 1) with x_out != NULL the
 * updated parameters are written to the client matrix instead of back to the
 * blocks: block j of client k lands at x_out + k*out_ld + out_offsets[j]
 * (the trainer's "training order" client matrix, run_experiments.py:238),
 * negated for clients k < nneg (sign-flip attackers, model_poisoning.py:
 * 274-276).  This folds the round's export pass into the optimizer.
 * Clip norm from producer partials: blocks with block_normed[j] != 0 are left
 * out of the optimizer's own sum-of-squares pass; their squares come as fp64
 * partials extra_sq[k*n_extra + i], i < n_extra (e.g. written by
 * flr_conv2d_bwd_weight_t_sq), summed per client in a fixed order. */
int flr_clip_sgd_step_blocked_x(float* const* x_blocks, const float* const* g_blocks,
                                float* const* m_blocks, const int64_t* block_numel,
                                const int64_t* block_client_stride, int64_t nblocks,
                                int64_t K, float lr, float momentum, float weight_decay,
                                float max_norm, int first_step, float* x_out,
                                const int64_t* out_offsets, int64_t out_ld, int64_t nneg,
                                const uint8_t* block_normed, const double* extra_sq,
                                int64_t n_extra, float* norms_out, void* workspace,
                                size_t workspace_bytes, void* stream);
/* flr_clip_sgd_step_blocked_x whose FIRST step reads every client's parameters
 * of block j from one shared vector, x_src + src_offsets[j] (the global model
 * all clients start from, so no per-client copy of it is loaded; offset < 0:
 * the block reads x_blocks[j]); the update still goes to x_blocks (or x_out on
 * a last step, where src_offsets[j] must equal out_offsets[j]).  x_src NULL:
 * flr_clip_sgd_step_blocked_x. */
int flr_clip_sgd_step_blocked_src(float* const* x_blocks, const float* const* g_blocks,
                                  float* const* m_blocks, const int64_t* block_numel,
                                  const int64_t* block_client_stride, int64_t nblocks, int64_t K,
                                  float lr, float momentum, float weight_decay, float max_norm,
                                  int first_step, float* x_out, const int64_t* out_offsets,
                                  int64_t out_ld, int64_t nneg, const uint8_t* block_normed,
                                  const double* extra_sq, int64_t n_extra, const float* x_src,
                                  const int64_t* src_offsets, float* norms_out, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* flr_clip_sgd_step_blocked_src in two phases, so the update can overlap
 * other work (the native trainers run it on a side stream, parameter group by
 * parameter group, under the next local step's forward):
 *   FLR_SGD_PHASE_NORM   the clip norms and coefficients of ALL the blocks
 *                        passed (per-client, into the workspace; norms_out);
 *   FLR_SGD_PHASE_UPDATE the clip + momentum + parameter update of the blocks
 *                        passed (any subset, any order), reading the
 *                        coefficients a NORM phase left in the same workspace;
 *   FLR_SGD_PHASE_ALL    both (= flr_clip_sgd_step_blocked_src).
 * The update is elementwise: splitting it over calls changes no bit. */
#define FLR_SGD_PHASE_NORM 1
#define FLR_SGD_PHASE_UPDATE 2
#define FLR_SGD_PHASE_ALL 3
int flr_clip_sgd_step_phase(float* const* x_blocks, const float* const* g_blocks, float* const* m_blocks,
                            const int64_t* block_numel, const int64_t* block_client_stride,
                            int64_t nblocks, int64_t K, float lr, float momentum, float weight_decay,
                            float max_norm, int first_step, float* x_out, const int64_t* out_offsets,
                            int64_t out_ld, int64_t nneg, const uint8_t* block_normed,
                            const double* extra_sq, int64_t n_extra, const float* x_src,
                            const int64_t* src_offsets, float* norms_out, int phase, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- a2: client-batched 2-D convolution (bias-free, as in the conv blocks)
 * Replaces nn.Conv2d forward/backward for every client of a GPU at once
 * (image branch, src/models/cub200_cnn.py:71-77 template).  Layouts:
 *   x  [K][Cin][B][H][W]   (client-channel major: for one (client, channel)
 *                           the B*H*W pixels the GEMM walks are contiguous)
 *   w  [K][Cout][Cin][KH][KW]
 *   y  [K][Cout][B][Ho][Wo], Ho = (H + 2 pad - KH) / stride + 1
 * fp32 in, fp32 accumulate: each operand split into three bf16 terms, six
 * products per k-step on v_mfma_f32_32x32x16_bf16 (per-product error a few
 * 2^-24 |a b|, the size of an fp32 product's rounding); FLR_GEMM=f32 selects
 * the exact-fp32 v_mfma_f32_32x32x2_f32.  bwd_data writes dx, bwd_weight
 * writes dw (both overwrite).  Kernel taps that only read zero padding are
 * skipped (their dw is written as exact zeros).  The workspace (optional,
 * size from flr_conv2d_workspace) enables deterministic split-K for long
 * reductions; without it the kernels run unsplit. */
size_t flr_conv2d_workspace(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                            int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                            int64_t pad);
int flr_conv2d_fwd(const float* x, const float* w, float* y, int64_t K, int64_t B,
                   int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH,
                   int64_t KW, int64_t stride, int64_t pad, void* workspace,
                   size_t workspace_bytes, void* stream);
int flr_conv2d_bwd_data(const float* dy, const float* w, float* dx, int64_t K,
                        int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                        int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                        void* workspace, size_t workspace_bytes, void* stream);
int flr_conv2d_bwd_weight(const float* x, const float* dy, float* dw, int64_t K,
                          int64_t B, int64_t Cin, int64_t H, int64_t W,
                          int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                          int64_t pad, void* workspace, size_t workspace_bytes,
                          void* stream);
/* flr_conv2d_bwd_weight given the workspace of the flr_conv2d_fwd call that
 * consumed the same x (and has not been reused since): when that forward took
 * the explicit-im2col path (short reductions: the 7x7 stem), its column matrix
 * heads the workspace and the weight gradient reads it instead of rebuilding
 * it.  Otherwise identical to flr_conv2d_bwd_weight. */
int flr_conv2d_bwd_weight_reuse(const float* x, const float* dy, float* dw, int64_t K,
                                int64_t B, int64_t Cin, int64_t H, int64_t W,
                                int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                int64_t pad, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ---- a5: cross-entropy forward + backward ------------------------------
 * Replaces nn.CrossEntropyLoss() (mean over each client's batch;
 * run_experiments.py:186, 232) for K clients × B rows × C classes:
 *   loss[k] = mean_b (logsumexp(z_kb) - z_kb[y_kb]);
 *   dlogits = (softmax(z) - onehot(y)) / B.
 * logits/dlogits: device fp32 [K*B, C]; labels: device int64 [K*B];
 * loss: device fp32 [K]; loss_rows: device fp32 [K*B] scratch.
 */
int flr_cross_entropy(const float* logits, const int64_t* labels, int64_t K,
                      int64_t B, int64_t C, float* loss, float* dlogits,
                      float* loss_rows, void* stream);
/* out[c] = (sum_r X[r][c]) / R, the sum sequential in fp64: each client's
 * reported training loss, the mean of its per-step losses (fl_client.py:143-149). */
int flr_mean_rows(const float* X, int64_t R, int64_t C, float* out, void* stream);
/* d[k, b, c] *= gk[k]  (chain rule for a per-client upstream gradient). */
int flr_scale_client_rows(float* d, const float* gk, int64_t K, int64_t B,
                          int64_t C, void* stream);

/* Tap-major variants (the training engine's conv layout when Cin and Cout are
 * multiples of 64): w_t / dw_t are [K][KH][KW][Cin][Cout] per client, i.e.
 * torch's [Cout][Cin][KH][KW] permuted (0, 2, 3, 1) per client.  Same
 * activations, outputs and semantics as flr_conv2d_fwd / _bwd_data /
 * _bwd_weight; FLR_ERR_UNSUPPORTED when the channel counts do not qualify
 * (flr_conv2d_tap_major_ok).  Workspace (optional, split-K) from
 * flr_conv2d_t_workspace. */
int flr_conv2d_tap_major_ok(int64_t Cin, int64_t Cout);
size_t flr_conv2d_t_workspace(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                              int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                              int64_t pad);
int flr_conv2d_fwd_t(const float* x, const float* w_t, float* y, int64_t K, int64_t B,
                     int64_t Cin, int64_t H, int64_t W, int64_t Cout, int64_t KH,
                     int64_t KW, int64_t stride, int64_t pad, void* workspace,
                     size_t workspace_bytes, void* stream);
int flr_conv2d_bwd_data_t(const float* dy, const float* w_t, float* dx, int64_t K,
                          int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                          int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                          void* workspace, size_t workspace_bytes, void* stream);
/* dx = dgrad + add (one rounding per element; add in dx's layout, NULL: none):
 * the residual block's two input-gradient paths summed in the dgrad epilogue,
 * the value autograd's accumulation of the conv path and the shortcut path
 * gives (the reference's BasicBlock backward, torchvision resnet18).  add may
 * be dx itself (in-place accumulation, dx += dgrad): the stride-parity classes
 * no kernel tap reaches are then skipped (a strided 1x1 shortcut writes only
 * its one class instead of zeros over the other three). */
int flr_conv2d_bwd_data_t_add(const float* dy, const float* w_t, const float* add,
                              float* dx, int64_t K, int64_t B, int64_t Cin, int64_t H,
                              int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                              int64_t stride, int64_t pad, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The forward and the input gradient with w_stride floats between clients'
 * weights (KH*KW*Cin*Cout: the per-client layout above; 0: every client reads
 * the one copy at w_t — the first local step, when every client still holds
 * the global model, needs no per-client copy of it). */
int flr_conv2d_fwd_t_ex(const float* x, const float* w_t, int64_t w_stride, float* y,
                        int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                        int64_t KH, int64_t KW, int64_t stride, int64_t pad, void* workspace,
                        size_t workspace_bytes, void* stream);
int flr_conv2d_bwd_data_t_ex(const float* dy, const float* w_t, int64_t w_stride,
                             const float* add, float* dx, int64_t K, int64_t B, int64_t Cin,
                             int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                             int64_t stride, int64_t pad, void* workspace,
                             size_t workspace_bytes, void* stream);
/* flr_conv2d_bwd_data_t_ex with the residual block's strided 1x1 shortcut folded
 * in: dx = dgrad(conv) [+ add], then dx += dgrad(shortcut) where the shortcut is
 * the 1x1 convolution of the same K, B, Cin, H, W and stride, pad 0, Cout_ds
 * output channels, gradient dy_ds [K][Cout_ds][B][Ho][Wo] and tap-major weights
 * w_ds (w_ds_stride floats between clients, 0: one shared copy).  The values are
 * those of the two calls flr_conv2d_bwd_data_t_ex(conv, add, dx) then
 * flr_conv2d_bwd_data_t_ex(shortcut, add = dx, dx), bit for bit.  dy_ds and w_ds
 * NULL: no shortcut (flr_conv2d_bwd_data_t_ex itself).
 *
 * Stride 2 with H and W even may run as ONE launch (the fused form): a workgroup
 * walks the four stride-parity classes of its pixels (and the shortcut) with the
 * per-class kernel's K-loop, sums each class's split-K ranges in the reduce pass's
 * order without writing partials, and stores whole rows of dx.  The knob
 * FLR_DGRAD_FUSED (flr_set_knob, read per launch) chooses: 0 the per-class
 * launches, 1 the fused form wherever supported, unset the per-shape preference
 * (flr_conv2d_dgrad_fused_preferred).  Either form writes the same bits; every
 * other geometry, a dx that is not 8-byte aligned, and an in-place call
 * (add == dx) with a class no tap reaches take the per-class launches. */
int flr_conv2d_bwd_data_t_sc(const float* dy, const float* w_t, int64_t w_stride,
                             const float* add, float* dx, int64_t K, int64_t B, int64_t Cin,
                             int64_t H, int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                             int64_t stride, int64_t pad, const float* dy_ds,
                             const float* w_ds, int64_t w_ds_stride, int64_t Cout_ds,
                             void* workspace, size_t workspace_bytes, void* stream);
/* 1 when the geometry has a fused form (tap-major, stride 2, H and W even). */
int flr_conv2d_dgrad_fused_supported(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                                     int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                     int64_t pad);
/* 1 when a call of this geometry (shortcut != 0: with a folded shortcut) runs
 * fused under the current FLR_DGRAD_FUSED setting: supported, and the knob is 1
 * or unset with the shape among those measured faster fused on MI355X. */
int flr_conv2d_dgrad_fused_preferred(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                                     int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                     int64_t pad, int shortcut);
/* The split-K count of stride-parity class cls_index (row-major over (ih % stride,
 * iw % stride)) of the data gradient given a workspace of workspace_bytes: the
 * per-class launch's count, which the fused form reproduces in-register.
 * 0: no such class. */
int flr_conv2d_dgrad_class_splits(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                                  int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                  int64_t pad, int cls_index, size_t workspace_bytes);
/* 1 when flr_conv2d_fwd_t_ex (dgrad == 0) or flr_conv2d_bwd_data_t_ex (dgrad != 0)
 * runs this geometry on the resident-B kernel: the tile's activation operand split
 * into bf16 term images once and kept in LDS across the kernel taps, only the
 * weights staged per K-tile.  Taken for stride-1 "same" convolutions with 64
 * channels on both sides whose H*W divides 128 and whose default split-K count is
 * 1 (ResNet-18's layer1); the bits are the default kernel's.  The knob
 * FLR_CONV_RESIDENT=0 (flr_set_knob, read per launch) turns the form off: 0 then. */
int flr_conv2d_resident_ok(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                           int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                           int64_t pad, int dgrad);
/* zero_dead_taps: write the dead taps' slabs of dw_t as zeros (1) or leave
 * them untouched (0: the caller never reads them, see
 * flr_clip_sgd_step_blocked). */
int flr_conv2d_bwd_weight_t(const float* x, const float* dy, float* dw_t, int64_t K,
                            int64_t B, int64_t Cin, int64_t H, int64_t W,
                            int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                            int64_t pad, int zero_dead_taps, void* workspace,
                            size_t workspace_bytes, void* stream);
/* The same weight gradient, plus the clip norm's partial sums of squares
 * (a6, run_experiments.py:234): fp64 sums over fixed parts of client k's
 * live-tap gradient at sq[k*sq_ld + i], i < the slot count
 * flr_conv2d_bwd_weight_t_sq_slots returns for the geometry (<= sq_ld).
 * The parts depend on the per-client shape only, never on K.  Needs the
 * full flr_conv2d_t_workspace (FLR_ERR_WORKSPACE otherwise). */
int64_t flr_conv2d_bwd_weight_t_sq_slots(int64_t K, int64_t B, int64_t Cin, int64_t H,
                                         int64_t W, int64_t Cout, int64_t KH, int64_t KW,
                                         int64_t stride, int64_t pad);
int flr_conv2d_bwd_weight_t_sq(const float* x, const float* dy, float* dw_t, int64_t K,
                               int64_t B, int64_t Cin, int64_t H, int64_t W,
                               int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                               int64_t pad, int zero_dead_taps, double* sq, int64_t sq_ld,
                               void* workspace, size_t workspace_bytes, void* stream);
/* 1 when flr_conv2d_bwd_weight_t[_sq] runs this geometry on the resident weight-
 * gradient kernel: a workgroup owns three taps of one split-K part, stages x and dy
 * once per 64-pixel chunk of whole images as transposed bf16 term images, and reads
 * each tap's x fragment at the shifted pixel row (or a zero row for padding).  Taken
 * for stride-1 "same" convolutions with 64 channels on both sides whose H*W divides
 * 64 and is a multiple of 4, with a multiple of three live taps (ResNet-18's
 * layer1); a split-K part that begins inside an image is handled.  Split count,
 * partials, clip-norm slots and bits are the default kernel's.  The knob
 * FLR_WGRAD_RESIDENT=0 (flr_set_knob, read per launch) turns the form off: 0 then. */
int flr_conv2d_wgrad_resident_ok(int64_t K, int64_t B, int64_t Cin, int64_t H, int64_t W,
                                 int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                                 int64_t pad);

/* ---- a1 / a8 / a15: round-boundary layout moves of the training state ----
 * flr_broadcast_rows: dst[k*dst_stride + i] = src[i] (load_global: every
 * client starts from the global model, run_experiments.py:203).
 * flr_copy_rows: dst[k*dst_stride + i] = src[k*src_stride + i] (parameter
 * block -> client-matrix columns, run_experiments.py:238 + krum.py:55-57).
 * flr_tap_major_to_torch: w_t [K][KK][Cin][Cout] -> torch order
 * [Cout][Cin][KK] at dst + k*dst_stride (KK <= 9). */
int flr_broadcast_rows(const float* src, int64_t n, float* dst, int64_t K,
                       int64_t dst_stride, void* stream);
/* flr_broadcast_rows with rows k < nneg written as -src (the attackers' copy
 * of a range the optimizer never updates, e.g. dead conv taps). */
int flr_broadcast_rows_neg(const float* src, int64_t n, float* dst, int64_t K,
                           int64_t dst_stride, int64_t nneg, void* stream);
int flr_copy_rows(const float* src, int64_t src_stride, int64_t n, float* dst,
                  int64_t dst_stride, int64_t K, void* stream);
int flr_tap_major_to_torch(const float* w_t, int64_t K, int64_t KK, int64_t Cin,
                           int64_t Cout, float* dst, int64_t dst_stride, void* stream);
/* The same two exports with rows k < nneg written negated: the sign-flip
 * attackers' submitted update (model_poisoning.py:274-276, applied after
 * training as malicious_client.py:103-115) folded into the export pass. */
int flr_copy_rows_neg(const float* src, int64_t src_stride, int64_t n, float* dst, int64_t dst_stride, int64_t K,
                      int64_t nneg, void* stream);
int flr_tap_major_to_torch_neg(const float* w_t, int64_t K, int64_t KK, int64_t Cin, int64_t Cout, float* dst,
                               int64_t dst_stride, int64_t nneg, void* stream);

/* ---- §8(f): per-client norms and weighted row combinations ---------------
 * Building blocks of GradientClippingDefense / NormBoundingDefense /
 * DPSGDDefense (src/defenses/differential_privacy.py:74-164, 223-334) and
 * GeometricMedianDefense (src/defenses/trimmed_mean.py:177-265).
 * flr_row_norms: out[i] = ||X_i - center||_2 (type 0) or ||.||_inf (type 1),
 * center optional [P]; differences rounded to fp32, squares summed in fp64 in
 * a fixed order.  Workspace: flr_row_norms_workspace(K) bytes.
 * flr_weighted_rows: out = (sum_j fl(fl(X[rows[j]] * scales[j]) * weights[j]))
 * / divisor, sequential in j (rows NULL = all K rows in order, m = K; scales
 * NULL = 1).  weights/scales are device float arrays of length m. */
size_t flr_row_norms_workspace(int64_t K);
int flr_row_norms(const float* X, int64_t K, int64_t P, int64_t ldx,
                  const float* center, int type, double* out, void* workspace,
                  size_t workspace_bytes, void* stream);
/* out[i] = X_i . v (fp64 sum of exact products); workspace as flr_row_norms.
 * FLTrust's torch.dot (src/defenses/fltrust.py:176). */
int flr_row_dots(const float* X, int64_t K, int64_t P, int64_t ldx, const float* v,
                 double* out, void* workspace, size_t workspace_bytes, void* stream);
int flr_weighted_rows(const float* X, int64_t K, int64_t P, int64_t ldx,
                      const int32_t* rows, int64_t m, const float* weights,
                      const float* scales, float divisor, float* out,
                      void* stream);

/* ---- a3: GRU recurrence, pointwise gate math per time step ----------------
 * Replaces the per-step cell of nn.GRU (torch gate order r, z, n;
 * h' = (h - n) * z + n), used by the text branch of the multimodal model.
 * Layouts: gi [K][B][T][3H], gh [K][B][3H] (= h_t W_hh^T + b_hh),
 * hseq [K][T+1][B][H], gates [K][T][B][4][H] (r, z, n, h_n),
 * dgh [K][T][B][3H], dgi [K][B][T][3H], dh / dh_direct [K][B][H].
 * fwd_step reads hseq[:, t] and writes hseq[:, t+1] and gates[:, t];
 * bwd_step takes dh = dL/dh_{t+1} and writes dgh[:, t], dgi[:, :, t] and
 * dh_direct (the z-gate path of dL/dh_t; the caller adds dgh[:, t] W_hh). */
int flr_gru_fwd_step(const float* gi, const float* gh, float* hseq, float* gates,
                     int64_t K, int64_t B, int64_t T, int64_t H, int64_t t,
                     void* stream);
int flr_gru_bwd_step(const float* dh, const float* gates, const float* hseq,
                     float* dgh, float* dgi, float* dh_direct, int64_t K,
                     int64_t B, int64_t T, int64_t H, int64_t t, void* stream);
/* Fused recurrence steps (B <= 32): one launch per time step instead of a
 * batched GEMM plus a gate kernel.  flr_gru_fwd_fused: gh = h_t W_hh^T + b_hh
 * (whhP = W_hh [K][3H][H] packed by flr_gru_pack(NG=3, C=H, trans=0), bhh
 * [K][3H]) and the gate math of flr_gru_fwd_step in the GEMM's epilogue.
 * flr_gru_bwd_fused (t >= 1): dh_t = dh_direct + dgh[:, t] W_hh (whhTP = W_hh^T
 * packed by flr_gru_pack(NG=1, C=3H, trans=1)), then flr_gru_bwd_step's math
 * for step t - 1 with dy = dh_t (dh_direct rewritten in place); dh0 (optional,
 * [K][B][H]) receives dh_t.  Same products as the batched GEMM (bf16x6 on MFMA,
 * fp32 accumulate), a different reduction order. */
int flr_gru_fwd_fused(const float* gi, const float* whhP, const float* bhh, float* hseq, float* gates, int64_t K,
                      int64_t B, int64_t T, int64_t H, int64_t t, void* stream);
int flr_gru_bwd_fused(const float* whhTP, const float* gates, const float* hseq, float* dgh, float* dgi,
                      float* dh_direct, float* dh0, int64_t K, int64_t B, int64_t T, int64_t H, int64_t t,
                      void* stream);
/* The fused steps with shared_w = 1: every client reads the ONE packed copy at
 * whh / whhT (flr_gru_pack with K = 1): the first local step, when all clients
 * still hold the global W_hh.  shared_w = 0: the calls above. */
int flr_gru_fwd_fused_ex(const float* gi, const float* whh, int shared_w, const float* bhh,
                         float* hseq, float* gates, int64_t K, int64_t B, int64_t T, int64_t H,
                         int64_t t, void* stream);
int flr_gru_bwd_fused_ex(const float* whhT, int shared_w, const float* gates, const float* hseq,
                         float* dgh, float* dgi, float* dh_direct, float* dh0, int64_t K,
                         int64_t B, int64_t T, int64_t H, int64_t t, void* stream);
/* The whole recurrence in one launch per pass: one workgroup per client loops
 * over the time steps, h_t / dgh_t handed from step to step through LDS.
 * flr_gru_fwd_seq is flr_gru_fwd_fused_ex for t = 0 .. T-1 (reads hseq[:, 0],
 * writes hseq[:, 1..T] and gates); flr_gru_bwd_seq is flr_gru_bwd_step at
 * T-1 from dh = dL/dh_T, then flr_gru_bwd_fused_ex for t = T-1 .. 1 (writes
 * all of dgh and dgi; dh_direct as the last step leaves it; dh0, optional,
 * as the t = 1 call writes it, so only when T >= 2).  Results are the per-step
 * default form's bit for bit.  Shapes: B <= 32, H % 32 == 0, H <= 256, any
 * T >= 1; otherwise, and with FLR_GRU_SEQ=0 (flr_set_knob, read per call),
 * FLR_ERR_UNSUPPORTED and nothing is written: use the per-step calls.
 * flr_gru_seq_supported: 1 when the two would run this shape now, else 0.
 * flr_gru_seq_preferred: 1 when a caller with both forms should take this one
 * (supported, and K * H/32 > 768, from where it measured faster than the
 * per-step launches on MI355X; FLR_GRU_SEQ=1: wherever supported), else 0.
 * flr_gru_zero_h0: hseq[:, 0] = 0, the one slot the forward does not write. */
int flr_gru_fwd_seq(const float* gi, const float* whhP, int shared_w, const float* bhh, float* hseq, float* gates,
                    int64_t K, int64_t B, int64_t T, int64_t H, void* stream);
int flr_gru_bwd_seq(const float* whhTP, int shared_w, const float* gates, const float* hseq, const float* dh,
                    float* dgh, float* dgi, float* dh_direct, float* dh0, int64_t K, int64_t B, int64_t T,
                    int64_t H, void* stream);
int flr_gru_seq_supported(int64_t K, int64_t B, int64_t T, int64_t H);
int flr_gru_seq_preferred(int64_t K, int64_t B, int64_t T, int64_t H);
int flr_gru_zero_h0(float* hseq, int64_t K, int64_t B, int64_t T, int64_t H, void* stream);
/* Pack a per-client weight into the fused kernels' MFMA-fragment order: the
 * [NG*H][C] operand (trans = 0: w is [NG*H][C]; trans = 1, NG = 1: w is [C][H]
 * and the operand is its transpose) in 32-row blocks x 16-deep k-steps, each
 * (block, k-step) 512 floats (two 1 KB wave loads), zero-padded.  wp holds
 * K * NG * ceil(H/32) * ceil(C/16) * 512 floats. */
int flr_gru_pack(const float* w, int64_t K, int64_t NG, int64_t H, int64_t C, int trans, float* wp, void* stream);

/* ---- a2: per-client BatchNorm (train mode) + fused residual add / ReLU ----
 * Replaces nn.BatchNorm2d(train) [+ identity add] [+ ReLU] of the conv blocks.
 * x, y, residual: [B][KC][HW] (kc = client*C + channel; the engine's
 * [K][C][B][H][W] activations are passed as B = 1, HW = B*H*W), gamma/beta/mean/
 * invstd: [KC].  fwd: y = act(x*alpha + (beta - mean*alpha) [+ residual]),
 * alpha = gamma/sqrt(var + eps), batch statistics over B*HW, act = ReLU if
 * relu != 0.  bwd: g = dy * (y > 0) if relu else dy; writes dx, dgamma,
 * dbeta, and dresidual = g when dresidual != NULL. */
int flr_batchnorm_fwd(const float* x, const float* gamma, const float* beta,
                      const float* residual, float* y, float* mean, float* invstd,
                      int64_t B, int64_t KC, int64_t HW, float eps, int relu,
                      void* stream);
int flr_batchnorm_bwd(const float* dy, const float* x, const float* y,
                      const float* gamma, const float* mean, const float* invstd,
                      float* dx, float* dgamma, float* dbeta, float* dresidual,
                      int64_t B, int64_t KC, int64_t HW, int relu, void* stream);
/* The ResNet stem's BatchNorm + ReLU + 3x3/2 pad-1 max-pool as one kernel each
 * way (torchvision resnet18 stem: bn1 -> relu -> maxpool), per (client,
 * channel) plane of NI images of H x W: the same values as flr_batchnorm_fwd
 * (relu, no residual) followed by flr_maxpool2d_fwd, and as flr_maxpool2d_bwd
 * followed by flr_batchnorm_bwd (relu; the mask recomputed from x, beta and
 * the saved statistics), without the BN output / its gradient in HBM.
 * y_pool / dy_pool: [KC][NI][H/2][W/2], argmax: 1-byte window offsets as
 * flr_maxpool2d_fwd's.  Shapes: H = W = 16, NI = 16 or 32 (the stem at 32 x 32
 * inputs, batch 16 / 32); else FLR_ERR_UNSUPPORTED (use the two-kernel form). */
int flr_batchnorm_relu_maxpool_fwd(const float* x, const float* gamma, const float* beta,
                                   float* y_pool, uint8_t* argmax, float* mean, float* invstd,
                                   int64_t KC, int64_t NI, int64_t H, int64_t W, float eps,
                                   void* stream);
int flr_maxpool_relu_batchnorm_bwd(const float* dy_pool, const uint8_t* argmax, const float* x,
                                   const float* gamma, const float* beta, const float* mean,
                                   const float* invstd, float* dx, float* dgamma, float* dbeta,
                                   int64_t KC, int64_t NI, int64_t H, int64_t W, void* stream);

/* ---- a3 / a4: batched dense GEMM (text branch, late-fusion MLP) ------------
 * Replaces the nn.Linear / nn.GRU matrix products of the text branch and the
 * fusion head (src/models/cub200_cnn.py:80-93, 107-117 template) for every
 * client at once:
 *   C_k[m][n] = (bias_k[n] or add_k[m][n] or 0) + sum_r A_k(m, r) B_k(n, r)
 * A(m, r) at A + k*a_k + m*a_m + r*a_r (B, C likewise; any strides, so
 * transposed operands are views); bias: NULL or [batch][bias_k] row vectors;
 * add: NULL or a C-shaped addend (may alias C).  Same MFMA tiles as the
 * convolutions (three-term bf16 split, fp32 accumulate; FLR_GEMM=f32: exact-fp32
 * MFMA); split-K chosen from (M, N, R) alone, so every client's result is
 * independent of the batch count.  Workspace (optional, split-K partials): flr_bgemm_workspace.
 * flr_sum_rows: out[k][n] = sum_m X[k][m][n] (bias gradients; eight interleaved
 * partial sums in a fixed order, deterministic). */
size_t flr_bgemm_workspace(int64_t batch, int64_t M, int64_t N, int64_t R);
/* flr_bgemm with a fused epilogue, applied per output element after the
 * bias / addend (and after the split-K reduction):
 *   pre (optional, C-shaped) <- v;  v <- act(v);  v <- v * mul (optional);  C <- v
 * act: FLR_ACT_NONE, _RELU, _GELU (exact erf, torch's nn.GELU()), _TANH; the
 * backward modes multiply the incoming gradient v by the activation's
 * derivative at aux (C-shaped, required): _DRELU (aux > 0, aux = the ReLU
 * input or output), _DGELU (aux = the GELU input), _DTANH (aux = the tanh
 * output).  mul / aux / pre share C's strides.  The late-fusion head's
 * ReLU + dropout mask, the transformer MLP's GELU and BERT's pooler tanh run
 * here instead of as separate elementwise passes. */
#define FLR_ACT_NONE 0
#define FLR_ACT_RELU 1
#define FLR_ACT_GELU 2
#define FLR_ACT_TANH 3
#define FLR_ACT_DRELU 4
#define FLR_ACT_DGELU 5
#define FLR_ACT_DTANH 6
int flr_bgemm_ex(const float* A, int64_t a_k, int64_t a_m, int64_t a_r, const float* B, int64_t b_k, int64_t b_n,
                 int64_t b_r, float* C, int64_t c_k, int64_t c_m, int64_t c_n, const float* bias, int64_t bias_k,
                 const float* add, int act, const float* mul, const float* aux, float* pre, int64_t batch,
                 int64_t M, int64_t N, int64_t R, void* workspace, size_t workspace_bytes, void* stream);
int flr_bgemm(const float* A, int64_t a_k, int64_t a_m, int64_t a_r, const float* B,
              int64_t b_k, int64_t b_n, int64_t b_r, float* C, int64_t c_k, int64_t c_m,
              int64_t c_n, const float* bias, int64_t bias_k, const float* add,
              int64_t batch, int64_t M, int64_t N, int64_t R, void* workspace,
              size_t workspace_bytes, void* stream);
int flr_sum_rows(const float* X, int64_t x_k, int64_t x_m, int64_t batch, int64_t M,
                 int64_t N, float* out, int64_t out_k, void* stream);
/* The same sum over M > 256 rows as fixed 256-row chunks reduced in chunk order
 * (a chunking that depends on M alone); workspace flr_sum_rows_workspace (0:
 * one pass, as flr_sum_rows). */
size_t flr_sum_rows_workspace(int64_t batch, int64_t M, int64_t N);
int flr_sum_rows_ex(const float* X, int64_t x_k, int64_t x_m, int64_t batch, int64_t M, int64_t N, float* out,
                    int64_t out_k, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a2: max pooling of the image branch (the stem's 3x3/2 pad-1 pool) ----
 * Replaces nn.MaxPool2d / F.max_pool2d on x [nplanes][H][W] (planes = B*K*C of
 * the grouped layout).  torch's CPU rule: first in-bounds element of the
 * row-major window scan with (v > max || isnan(v)) wins; argmax [nplanes][Ho][Wo]
 * holds its window offset kh*KW + kw.  bwd: dx[e] = sum of dy over the windows
 * whose argmax is e, in output raster order (overwrites dx). */
int flr_maxpool2d_fwd(const float* x, float* y, uint8_t* argmax, int64_t nplanes, int64_t H,
                      int64_t W, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                      void* stream);
int flr_maxpool2d_bwd(const float* dy, const uint8_t* argmax, float* dx, int64_t nplanes,
                      int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t stride,
                      int64_t pad, void* stream);

/* ---- §8(f): per-round evaluation of the global model (forward only) -------
 * Replaces evaluate_model / compute_attack_success_rate /
 * compute_label_flip_asr (src/utils/metrics.py:14-157).
 * flr_batchnorm_infer: model.eval() BatchNorm — running statistics instead of
 * batch statistics — with the optional residual add and ReLU of the training
 * kernel; x, residual, y [KC][HW] (one contiguous plane per (client, channel)),
 * gamma / beta / running_mean / running_var [KC].
 * flr_classify_rows: logits [R][C] -> pred[r] = first index of the maximum
 * (torch.max(outputs, 1); NaN counts as the maximum) and, with labels,
 * loss_rows[r] = logsumexp(z_r) - z_r[label].  counts (int64[5], accumulated:
 * the caller zeroes them) += {pred == label, pred == target, label == source,
 * label == source && pred == label, label == source && pred == target}.
 * labels may be NULL (then only counts[1] is updated). */
int flr_batchnorm_infer(const float* x, const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var,
                        const float* residual, float* y, int64_t KC, int64_t HW, float eps,
                        int relu, void* stream);
int flr_classify_rows(const float* logits, const int64_t* labels, int64_t R, int64_t C,
                      int64_t target, int64_t source, int32_t* pred, float* loss_rows,
                      int64_t* counts, void* stream);

/* ---- a3 + C4/C5 encoders: embedding, LayerNorm, self-attention -------------
 * (csrc/train_xfmr.hip).  Every op is batched over the clients of a GPU;
 * client k's rows are the k-th run of rows_per_client rows (or N positions).
 *
 * flr_fill: p[0..n) = value (a kernel, so it replays inside HIP graphs).
 *
 * flr_embedding_fwd replaces nn.Embedding (the GRU branch's token embedding,
 * BERT's word / token-type / position embeddings summed in that order):
 *   out[k][n] = ((w0[k][ids0[k][n]] + w1[k][ids1[k][n]]) + w2[k][ids2[k][n]])
 * wj at wj + k*wj_k (row-major [Vj][E]), idsj at idsj + k*idsj_k (stride 0 =
 * the same ids for every client); w1 / w2 may be NULL.  An id outside
 * [0, Vj) yields a NaN row (the caller validates; nothing faults).
 * flr_embedding_bwd: dtable[k][v] = sum of dout[k][n] over the n with
 * ids[k][n] == v, in increasing n, from 0 — torch's CPU embedding backward
 * (index_add in index order), bit for bit.  zero_fill != 0 first zeroes the
 * whole [V][E] table of every client; rows no id touches are otherwise left
 * as they are.  N <= 4096; workspace flr_embedding_bwd_workspace(K, N).
 */
int flr_fill(float* p, int64_t n, float value, void* stream);
/* out[i] = dy[i] * act'(aux[i]) [* mul[i]] for the FLR_ACT_D* modes (the
 * activation backward where no GEMM epilogue can take it). */
int flr_act_bwd(const float* dy, const float* aux, const float* mul, int act, float* out, int64_t n, void* stream);
int flr_embedding_fwd(const float* w0, int64_t w0_k, int64_t V0, const int64_t* ids0, int64_t ids0_k,
                      const float* w1, int64_t w1_k, int64_t V1, const int64_t* ids1, int64_t ids1_k,
                      const float* w2, int64_t w2_k, int64_t V2, const int64_t* ids2, int64_t ids2_k,
                      int64_t K, int64_t N, int64_t E, float* out, void* stream);
size_t flr_embedding_bwd_workspace(int64_t K, int64_t N);
int flr_embedding_bwd(const float* dout, const int64_t* ids, int64_t ids_k, int64_t K, int64_t N, int64_t V,
                      int64_t E, float* dtable, int64_t dtable_k, int zero_fill, void* workspace,
                      size_t workspace_bytes, void* stream);

/* flr_layernorm_fwd replaces nn.LayerNorm(D, eps) over `rows` rows (row i at
 * x + i*ldx, gamma / beta [K][D] for client i / rows_per_client), with the
 * residual add of the encoder block fused in front:
 *   s = x [+ residual];  y = (s - mean) rstd gamma + beta,  rstd = 1/sqrt(var + eps)
 * (biased variance).  s_out (optional, needs residual) receives s; mean / rstd
 * [rows] are saved for the backward.  D % 4 == 0, D <= 1024.
 * flr_layernorm_bwd: ds = rstd (g dy - mean(g dy) - xh mean(g dy xh)) [+ dskip],
 * xh = (s - mean) rstd, written to dx; dgamma / dbeta [K][D] = the per-client
 * sums over rows of dy xh / dy (fixed-order partials over 64-row chunks).
 * Workspace flr_layernorm_bwd_workspace(K, rows_per_client, D). */
int flr_layernorm_fwd(const float* x, int64_t ldx, const float* residual, int64_t ldr, const float* gamma,
                      const float* beta, float* y, int64_t ldy, float* s_out, int64_t lds, float* mean, float* rstd,
                      int64_t rows, int64_t D, int64_t rows_per_client, float eps, void* stream);
size_t flr_layernorm_bwd_workspace(int64_t K, int64_t rows_per_client, int64_t D);
int flr_layernorm_bwd(const float* dy, int64_t lddy, const float* s, int64_t lds, const float* gamma,
                      const float* mean, const float* rstd, const float* dskip, int64_t ldk, float* dx, int64_t lddx,
                      float* dgamma, float* dbeta, int64_t K, int64_t rows_per_client, int64_t D, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ViT token sequence: x0 [K][B][P+1][D], row t of sequence (k, b) =
 * (t == 0 ? cls[k] : tok[k][b*P + t - 1]) + pos[k][t]  (the class token and
 * the patch projections plus the learned position embedding).  D % 4 == 0,
 * 16-B aligned operands. */
int flr_vit_tokens(const float* tok, const float* cls, const float* pos, int64_t K, int64_t B, int64_t P, int64_t D,
                   float* x0, void* stream);

/* Multi-head self-attention core (no mask) for KB = clients x batch
 * sequences of T <= 96 tokens, H heads of width head_dim = 64:
 *   qkv [KB*T][3*H*64] = the fused in-projection's output (q | k | v, heads
 *   concatenated inside each);  S = q k^T / 8;  P = softmax(S);  ctx = P v
 *   ctx [KB*T][H*64];  lse [KB][H][T] = the softmax log-normalisers (saved).
 * flr_attention_bwd recomputes P from lse and writes dqkv [KB*T][3*H*64]
 * (dq | dk | dv).  fp32 on the VALU, one workgroup per (sequence, head). */
int flr_attention_fwd(const float* qkv, int64_t KB, int64_t T, int64_t H, int64_t head_dim, float* ctx, float* lse,
                      void* stream);
int flr_attention_bwd(const float* qkv, const float* ctx, const float* dctx, const float* lse, int64_t KB, int64_t T,
                      int64_t H, int64_t head_dim, float* dqkv, void* stream);

/* ---- a1: the client plugin's local update, one C entry --------------------
 * Replaces the simulation's per-client loop (run_experiments.py:193-240) and
 * FLClient.fit / _train (fl_client.py:76-149) for K clients of the C2/C3
 * model family (ResNet image trunk + embedding / 1-layer GRU text branch +
 * late-fusion head; the module layout of flr.models.multimodal.MultimodalNet)
 * without torch: every client starts from `global` (P floats in the
 * reference's parameters() order), runs `steps` local steps (forward, mean
 * cross-entropy, backward, clip_grad_norm_(max_norm) when max_norm > 0,
 * SGD(lr, momentum, weight_decay) re-created per client, so momentum starts at
 * the first gradient), and writes its parameters() vector to row k of X
 * (X + k*ld, ld >= P; rows k < nneg negated: the sign-flip attackers,
 * model_poisoning.py:274-276).  loss_out[k] = the mean of the client's
 * per-step losses (fl_client.py:143-149); norms_out (optional [K]) receives
 * the last step's pre-clip gradient norms.  Inputs, device, per step s:
 * images [steps][K][B][C][H][W] f32, tokens [steps][K][B][T] int64, labels
 * [steps][K][B] int64, dropout_masks NULL or [steps][K][B][fusion] f32 (the
 * inverted-dropout multipliers).  The same kernel schedule as the Python
 * trainer (flr.train.ClientBatchTrainer), so both give the same bits.  All
 * state lives in the workspace (flr_train_clients_workspace); image_size must
 * bring the trunk to a 1x1 map (32 for the four stride-2 stages).  The text
 * branch (embedding + GRU, forward and backward) and the convolutions' weight
 * gradients run on two per-device streams, forked from and joined to `stream`
 * by events inside the call (graph-capturable; created by
 * flr_train_clients_workspace, outside any capture): one training call per
 * device at a time.  FLR_TEXT_STREAM=0 / FLR_WGRAD_STREAM=0 keep that work on
 * `stream`; the results are the same bits either way. */
typedef struct flr_resnet_gru_spec {
  int64_t num_classes, image_size, in_channels;
  int64_t widths[4], blocks[4];  /* the four ResNet stages (BasicBlock) */
  int64_t vocab, seq_len, embed, hidden, fusion;
} flr_resnet_gru_spec;
int64_t flr_resnet_gru_num_params(const flr_resnet_gru_spec* spec);
size_t flr_train_clients_workspace(const flr_resnet_gru_spec* spec, int64_t K, int64_t B,
                                   int64_t steps);
int flr_train_clients(const flr_resnet_gru_spec* spec, const float* global, float* X,
                      int64_t ld, const float* images, const int64_t* tokens,
                      const int64_t* labels, const float* dropout_masks, int64_t steps,
                      int64_t K, int64_t B, float lr, float momentum, float weight_decay,
                      float max_norm, int64_t nneg, float* loss_out, float* norms_out,
                      void* workspace, size_t workspace_bytes, void* stream);
/* flags (flr_train_clients_ex):
 * FLR_TC_TRAIN_ORDER — `global` and X's rows are in TRAINING order: every
 *   tap-major conv weight (Cin, Cout multiples of 64) as [KH][KW][Cin][Cout]
 *   at its torch offset (flr_resnet_gru_reorder converts a P-vector either
 *   way).  The round engine's order (flr.round): Krum distances, row
 *   selections, coordinate-wise means and order statistics do not depend on a
 *   common coordinate permutation, so the last optimizer step writes X's rows
 *   directly (no export pass), the untrained dead-tap ranges are copied from
 *   `global`, and only the aggregated P-vector is permuted back.
 * FLR_TC_DEFER_DEAD (with FLR_TC_TRAIN_ORDER) — the dead-tap ranges are left
 *   unwritten; the caller writes them with flr_resnet_gru_fill_dead before
 *   anything reads them from X (the round engine: only when something other
 *   than its own Krum asks for the rows — the distances and the Multi-Krum
 *   mean read those taps from `global` itself,
 *   flr_pairwise_l2_reference_tap_dead / flr_rows_mean_dead).
 * Flag 0 is flr_train_clients. */
#define FLR_TC_TRAIN_ORDER 1u
#define FLR_TC_DEFER_DEAD 2u
int flr_train_clients_ex(const flr_resnet_gru_spec* spec, const float* global, float* X,
                         int64_t ld, const float* images, const int64_t* tokens,
                         const int64_t* labels, const float* dropout_masks, int64_t steps,
                         int64_t K, int64_t B, float lr, float momentum, float weight_decay,
                         float max_norm, int64_t nneg, float* loss_out, float* norms_out,
                         unsigned flags, void* workspace, size_t workspace_bytes, void* stream);
/* dst <- src (one P-vector) in training order (to_train = 1) or back in the
 * reference's parameters() order (0); src != dst. */
int flr_resnet_gru_reorder(const flr_resnet_gru_spec* spec, const float* src, float* dst,
                           int to_train, void* stream);
/* Parameters the optimizer updates: P minus the dead conv taps (taps that only
 * read zero padding at this image size; exact-zero gradients) when
 * weight_decay == 0, else P. */
int64_t flr_resnet_gru_live_params(const flr_resnet_gru_spec* spec, float weight_decay);
/* The dead-tap ranges of a training-order row ([off[r], off[r] + n[r]), whole
 * tap slabs of tap-major weights, ascending): their count, the first
 * min(count, cap) written (cap = 0: count only); -1 on a bad spec. */
int64_t flr_resnet_gru_dead_ranges(const flr_resnet_gru_spec* spec, float weight_decay, int64_t* off,
                                   int64_t* n, int64_t cap);
/* X's dead-tap ranges (rows 0 .. K-1, training order) <- gtrain's, rows
 * k < nneg negated: what flr_train_clients_ex writes last without
 * FLR_TC_DEFER_DEAD. */
int flr_resnet_gru_fill_dead(const flr_resnet_gru_spec* spec, float weight_decay, const float* gtrain,
                             float* X, int64_t ld, int64_t K, int64_t nneg, void* stream);

/* ---- a1 for the C4/C5 family: flr_train_vit_bert ---------------------------
 * The same client-plugin local update (run_experiments.py:193-240,
 * fl_client.py:76-149) for the ViT-S + BERT-mini late-fusion model
 * (flr.models.transformer.ViTBertNet: ViT patch embedding, class token,
 * position embedding, vit_depth pre-LN blocks, final LayerNorm; BERT word /
 * position / token-type embeddings, embedding LayerNorm, bert_depth post-LN
 * layers, tanh pooler; fc1 over [img | txt], ReLU, dropout mask, fc2), with no
 * torch: the kernel schedule of the Python trainer (flr.train.
 * ClientBatchTrainer), so both give the same bits.  Clients run in passes of
 * `chunk` clients (0: min(K, 32)); activations scale with the chunk, weights
 * (and momentum when steps > 1) with K.  Heads of width 64, <= 96 tokens per
 * sequence, widths <= 1024, B*seq_len <= 4096.  Inputs as flr_train_clients
 * (images [steps][K][B][C][S][S], tokens [steps][K][B][seq_len] int64 ids,
 * labels [steps][K][B], dropout_masks NULL or [steps][K][B][fusion]).  The
 * family has no training-layout change: X's rows are in parameters() order
 * with or without FLR_TC_TRAIN_ORDER, written by the last optimizer step.  The
 * ViT and BERT layers' weight and bias gradients run on the per-device
 * weight-gradient stream of flr_train_clients (created by
 * flr_train_vit_bert_workspace; forked and joined by events inside the call,
 * graph-capturable): one training call per device at a time;
 * FLR_WGRAD_STREAM=0 keeps them on `stream`, same bits. */
typedef struct flr_vit_bert_spec {
  int64_t num_classes, image_size, in_channels, patch;
  int64_t vit_dim, vit_depth, vit_heads, vit_mlp;
  int64_t vocab, seq_len, bert_dim, bert_depth, bert_heads, bert_ffn, bert_max_pos;
  int64_t fusion;
} flr_vit_bert_spec;
int64_t flr_vit_bert_num_params(const flr_vit_bert_spec* spec);
size_t flr_train_vit_bert_workspace(const flr_vit_bert_spec* spec, int64_t K, int64_t B, int64_t steps,
                                    int64_t chunk);
int flr_train_vit_bert(const flr_vit_bert_spec* spec, const float* global, float* X, int64_t ld,
                       const float* images, const int64_t* tokens, const int64_t* labels,
                       const float* dropout_masks, int64_t steps, int64_t K, int64_t B, float lr,
                       float momentum, float weight_decay, float max_norm, int64_t nneg, float* loss_out,
                       float* norms_out, unsigned flags, int64_t chunk, void* workspace,
                       size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLR_H */
