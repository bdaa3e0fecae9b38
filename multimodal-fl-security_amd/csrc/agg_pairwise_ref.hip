// a9, reference-exact mode — Krum distances bit-identical to the reference's
// fp32 `torch.norm(flat_i - flat_j).item()` (src/defenses/krum.py:89-97).
//
// The reference's norm on an fp32 CPU tensor accumulates (SURVEY.md App. C,
// probed on this image's torch; oracle/norm_ref.c restates it and
// tests/test_oracle.py pins it against torch.norm):
//   d = fl(x_i - x_j) elementwise;
//   8 fp32 lanes ("chains"), chain c = fma(d[8r+c], d[8r+c], chain c)
//   sequentially over the steps r = 0 .. R-1, R = P / 8;
//   s = chain 0 + chain 1 + ... + chain 7 (in that order);
//   the tail t >= 8R: while 4 or more remain, the next 4 as
//   s = s + fl(d[t] * d[t]) (separate multiply and add), then the last
//   0..3 as s = fma(d[t], d[t], s);
//   sqrt_f32(s) (correctly rounded), widened to fp64 by .item().
// Every fp32 operation here is that operation, in that order, so D is the
// reference's D bit for bit — no tolerance, no margin argument.
//
// Design.  The parallelism is fixed by the reference: K(K-1)/2 pairs x 8
// chains, each chain a sequential fma over R steps (65,024 chains of 1.475 M
// steps at C3): about one chain per lane of one wave per SIMD, so every step of
// a wave must be cheap and no wave may wait for another.
//  * Chain-major operands: a segment of X is first rewritten chain-major
//    (chain_transpose_kernel, Xc[k][c][s] = X[k][8(r0+s)+c], one read and one
//    write of the segment at HBM rate) so each chain's steps are contiguous.
//  * One wave per workgroup, one chain per lane: a wave holds 4 I rows (its
//    16-lane DPP rows) x 16 J rows (the lanes of a row) — 64 pairs — and
//    stages only the J rows it reads, so no wave waits at a barrier for
//    another (a shared 64-row J block behind a workgroup barrier cost 2.1 of
//    10.3 ms at C3: tools/gpu_r5_l.sh, profiles/r5_ref/).
//  * x_j per lane from LDS: per chunk of CS = 64 steps the wave stages its 16
//    (diagonal tiles: 20) J rows' 256-B chain pieces by LDS-DMA (one
//    global_load_lds_dwordx4 per 4 rows, XOR-swizzled 16-B slots so the
//    ds_read_b128 lane groups hit distinct banks) into a ring of NSTAGE stages
//    (DMA NSTAGE - 1 chunks ahead); each lane reads its row's 16 pieces with
//    ds_read_b128 one chunk ahead (two register buffers).
//  * x_i by DPP: lane L of each 16-lane row holds 4 steps of the chunk (one
//    16-B load per lane per chunk); step S reaches every lane of the row by a
//    row_newbcast of lane S / 4 folded into the subtraction (v_sub_f32_dpp).
//  * chain c = the XCD (blockIdx % 8): an XCD's L2 holds only its own chain's
//    streams.  40 KB of LDS per workgroup: four per CU, one wave per SIMD.
// Chains longer than the segment carry their partial sums in A between segments.
//  * Dead regions (flr_pairwise_l2_reference_tap_dead): a 3 x 3 block whose
//    dead taps equal +-g in every row is its own chain launch (run_chain_regions) over
//    two streams, the rows' live taps and one shared row of g + g (DeadPlan,
//    dead_chunk, ref_chain_dead_kernel); a pair of two rows of the same sign
//    skips the dead steps, fma(+0, +0, s) = s.
//
// Files: pwref_common.h (constants, tile numberings, TapBlock, DeadPlan),
// pwref_launch.h (one launcher per kernel family), agg_pairwise_ref_layout.hip
// (the chain-major rewrites), agg_pairwise_ref_dpp.hip (the DPP chain forms),
// agg_pairwise_ref_quad.hip (the throughput forms); here the finish kernel, the
// form plan (pick_form), the host planner and the C entry points.
#include <algorithm>
#include <cstring>

#include "pwref_launch.h"

namespace flr {
namespace pwref {

// D[i][j] = D[j][i] for the pairs of tiles [t0, t1): chains summed 0..7 in
// order, the tail, correctly rounded sqrt; the other pairs 0 (the ranks' parts
// are then summed: exactly one rank holds each pair), the diagonal 0.
__global__ void ref_finish_kernel(const float* __restrict__ A, int chains, const float* __restrict__ X,
                                  const TailCols tc, int K, int64_t P, int64_t ldx, int64_t R, int t0, int t1,
                                  double* __restrict__ D, const int* __restrict__ dflag, int nneg) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)K * K) return;
  const int i = (int)(idx / K), j = (int)(idx % K);
  if (i == j) {
    D[idx] = 0.0;
    return;
  }
  if (i > j) return;
  const int tile = tile_of_pair(i, j);
  double v = 0.0;
  if (tile >= t0 && tile < t1) {
    float s = 0.f;
    if (chains) {
      const int64_t kk = (int64_t)K * K, p = (int64_t)i * K + j;
      s = A[p];
#pragma unroll
      for (int c = 1; c < 8; ++c) s = add_rn(s, A[c * kk + p]);
    }
    const float* xi = X + (int64_t)i * ldx;
    const float* xj = X + (int64_t)j * ldx;
    int64_t t = R * 8;
    auto col = [&](int64_t c) { return tc.c[c - R * 8]; };
    if (t + 4 <= P)
      for (const int64_t e = t + 4; t < e; ++t) {
        const float d = xi[col(t)] - xj[col(t)];
        s = add_rn(s, mul_rn(d, d));
      }
    for (; t < P; ++t) {
      const float d = xi[col(t)] - xj[col(t)];
      s = __builtin_fmaf(d, d, s);
    }
    v = (double)sqrt_rn(s);
    // a dead region skipped this same-kind pair's dead steps: where a dead
    // value of g is not finite they are fl(g - g) = NaN, and so is the sum
    if (dflag && *dflag && ((i < nneg) == (j < nneg))) v = __builtin_nan("");
  }
  D[(int64_t)i * K + j] = v;
  D[(int64_t)j * K + i] = v;
}

}  // namespace pwref
}  // namespace flr

using namespace flr;
using namespace flr::pwref;

// The chain form of one call.  Dpp: ref_chain_kernel over any tile range.
// DppTwo: ref_chain2_kernel.  DeadRegions: Dpp with the blocks dead_block
// accepts as dead regions.  Quad*: the throughput forms over Xq segments — the
// workgroup form with x_i through LDS (the default) or in SGPRs, or one wave
// with 4 / 8 I rows.
enum class Form { Dpp, DppTwo, DeadRegions, QuadWgLds, QuadWgSgpr, QuadWave4, QuadWave8 };
static bool is_quad(Form f) { return f != Form::Dpp && f != Form::DppTwo && f != Form::DeadRegions; }
// the throughput forms hold K rounded up to 64 rows, and need more than one J block
static bool quad_reachable(int64_t K) { return K > QJ; }
static bool knob_is(const char* name, const char* prefix) {
  const char* e = flr::knob(name);
  return e && std::strncmp(e, prefix, std::strlen(prefix)) == 0;
}
// all_tiles: every pair in this call; dead: dead taps given (mask and g).
//  * the throughput forms: every pair, no tap-major blocks, K >= 480 (at least
//    two waves per SIMD); FLR_REF_SGPR=0 off, =1 from K > 64.
//    FLR_REF_SGPR_FORM=wave: the one-wave forms (A/B), FLR_REF_SGPR_ROWS=8 their
//    8-row one (default 4); FLR_REF_SGPR_FORM=sgpr: the workgroup form with
//    scalar x_i.
//  * the two-chain form, opt-in (FLR_REF_2I=1, from two super-blocks, K > 32):
//    measured -6 % at K=512 P=2M but +10 % at K=256 P=4M and +6 % on the C5
//    distances (profiles/r6_ref/two_chain_ab.json), so off by default.
//  * dead regions: unless FLR_REF_DEAD_SKIP=0.
static Form pick_form(int64_t K, int64_t ntaps, bool all_tiles, bool dead) {
  bool quad = all_tiles && ntaps == 0 && quad_reachable(K);
  if (quad && !knob_is("FLR_REF_SGPR", "1")) quad = K >= 480 && !knob_is("FLR_REF_SGPR", "0");
  if (quad) {
    if (knob_is("FLR_REF_SGPR_FORM", "wa")) return knob_is("FLR_REF_SGPR_ROWS", "8") ? Form::QuadWave8 : Form::QuadWave4;
    return knob_is("FLR_REF_SGPR_FORM", "s") ? Form::QuadWgSgpr : Form::QuadWgLds;
  }
  if (all_tiles && K > SB && knob_is("FLR_REF_2I", "1")) return Form::DppTwo;
  if (all_tiles && dead && !knob_is("FLR_REF_DEAD_SKIP", "0")) return Form::DeadRegions;
  return Form::Dpp;
}
// bytes per chain step of the widest segment any form may build for K rows
static int64_t widest_step_bytes(int64_t K) { return (quad_reachable(K) ? quad_rows(K) : K) * 8 * 4; }

extern "C" size_t flr_pairwise_l2_reference_workspace(int64_t K, int64_t P) {
  if (K < 1 || P < 0) return 0;
  const int64_t R = P / 8;
  size_t n = a_bytes(K);
  if (K < 2 || R == 0) return n;
  const int64_t per_step = widest_step_bytes(K);
  const int64_t nseg = (per_step * round_up_group(R) + XC_CAP - 1) / XC_CAP;
  const int64_t Rs = round_up_group((R + nseg - 1) / nseg);
  // dead regions (run_chain_regions), a one-GPU mode of moderate K: the dead
  // streams (one row: under P floats, and a few KB per block) and the padding
  // of up to 40 regions' streams to XC_GROUP steps
  const int64_t regions = K <= 512 ? 4 * P + (int64_t(4) << 20) + 40 * XC_GROUP * per_step : 0;
  return n + (size_t)(per_step * Rs + XC_SLACK + (quad_reachable(K) ? quad_slack(K) : 0) + regions);
}

extern "C" int flr_pairwise_l2_reference_tiles(int64_t K) {
  if (K < 2 || K > (1 << 15)) return 0;
  return ntiles_of((int)K);
}

// The transpose's waves for segment [r0, r0 + steps): every wave not inside
// one tap block (parse_taps: ascending and disjoint).
// Past WaveRuns::MAX runs the shortest gaps are bridged (those waves then
// also run; the tap kernel, launched after, rewrites their coordinates).
static WaveRuns wave_runs(const std::vector<TapBlock>& taps, int64_t r0, int64_t steps) {
  const int64_t nw = (steps + TW - 1) / TW;
  std::vector<std::pair<int64_t, int64_t>> v;  // [first, last + 1) wave runs
  size_t b = 0;
  for (int64_t w = 0; w < nw; ++w) {
    const int64_t u0 = 8 * (r0 + w * TW), u1 = u0 + 8 * TW;
    while (b < taps.size() && taps[b].end() <= u0) ++b;
    const bool inside = b < taps.size() && u0 >= taps[b].off && u1 <= taps[b].end();
    if (inside) continue;
    if (!v.empty() && v.back().second == w)
      v.back().second = w + 1;
    else
      v.push_back({w, w + 1});
  }
  while ((int)v.size() > WaveRuns::MAX) {  // bridge the shortest gap
    size_t best = 1;
    for (size_t i = 2; i < v.size(); ++i)
      if (v[i].first - v[i - 1].second < v[best].first - v[best - 1].second) best = i;
    v[best - 1].second = v[best].second;
    v.erase(v.begin() + (int64_t)best);
  }
  WaveRuns wr;
  wr.n = (int)v.size();
  wr.pre[0] = 0;
  for (int i = 0; i < wr.n; ++i) {
    wr.w0[i] = v[i].first;
    wr.pre[i + 1] = wr.pre[i] + (v[i].second - v[i].first);
  }
  return wr;
}

// A tap block that can run as a dead region: its plan, its live stream's steps
// per chain (whole periods, DeadPlan) and its dead stream in the workspace.
struct DeadBlock {
  bool fast = false;
  DeadPlan live{}, deadp{};  // the live taps' / the dead taps' nibbles
  int dm = 0;
  int64_t r0 = 0, S = 0;     // the block's chain steps [r0, r0 + S)
  int64_t Ll = 0, Lp = 0;    // live steps per chain, padded to XC_GROUP
  int64_t ldt = 0, toff = 0; // dead stream: floats per chain, offset of chain 0
};
static DeadBlock dead_block(const TapBlock& tb, uint64_t dm) {
  DeadBlock b;
  const int m = (int)(dm & 0x1ff);
  if (tb.kk != 9 || (m != DM_ONE && m != DM_FOUR) || tb.off % 8 != 0 || (tb.co * tb.ci * 9) % 8 != 0) return b;
  b.fast = true;
  b.dm = m;
  b.live.on = b.deadp.on = 1;
  for (int w = 0; w < 9; ++w) {  // a period's taps in the chain's order
    const int t = 8 - w;
    DeadPlan& p = ((m >> t) & 1) ? b.deadp : b.live;
    const int n = ((m >> t) & 1) ? b.deadp.nd++ : b.live.nl++;
    p.tap |= (uint64_t)t << (4 * n);
    p.rank |= (uint64_t)n << (4 * t);
  }
  b.live.nd = b.deadp.nd;
  b.deadp.nl = b.live.nl;
  b.r0 = tb.off / 8;
  b.S = tb.co * tb.ci * 9 / 8;
  const int64_t np = (b.S + 16) / 9;  // periods of virtual steps 0 .. S + 7
  b.Ll = np * b.live.nl;
  b.Lp = round_up_group(b.Ll);
  // the mixed waves run NSTD chunks per trip, CS / nl periods per chunk, and
  // prefetch NSTD - 1 chunks (1 KB per DMA) past the last
  const int64_t tch = CS / b.live.nl * b.deadp.nd, trip = (int64_t)NSTD * CS;
  b.ldt = ((b.Ll + trip - 1) / trip * NSTD + NSTD) * tch + 512;
  b.ldt = (b.ldt + 63) / 64 * 64;
  return b;
}
// One chain launch of a segment: a stretch of plain steps, or a dead region
struct Region {
  int64_t a, b;  // chain steps [a, b)
  int blk;       // the dead region's block, or -1
  int64_t pos;   // its streams' first step in the segment's workspace
};
// Segment [r0, r0 + steps) as regions, their streams packed at multiples of
// XC_GROUP steps: with `regions`, every block of db that may run as a dead
// region and lies whole inside the segment is one, the stretches between them
// plain; without, one plain stretch.  Returns the steps of workspace they take.
static int64_t plan_regions(const std::vector<DeadBlock>& db, int64_t r0, int64_t steps, bool regions,
                            std::vector<Region>& out) {
  out.clear();
  int64_t cur = r0, pos = 0;
  auto live = [&](int64_t a, int64_t b) {
    out.push_back({a, b, -1, pos});
    pos += round_up_group(b - a);
  };
  for (size_t b = 0; regions && b < db.size(); ++b) {
    const DeadBlock& d = db[b];
    if (!d.fast || d.r0 < cur || d.r0 + d.S > r0 + steps) continue;
    if (d.r0 > cur) live(cur, d.r0);
    out.push_back({d.r0, d.r0 + d.S, (int)b, pos});
    pos += d.Lp;
    cur = d.r0 + d.S;
  }
  if (cur < r0 + steps) live(cur, r0 + steps);
  return pos;
}

// The throughput forms: R chain steps of every pair in segments of Xq (K
// rounded up to 64 rows), per segment the block-major transpose and the chain
// kernel of `form`, continuing the sums in A (first: from 0).
static int run_quad_segments(Form form, const float* X, int64_t K, int64_t R, int64_t ldx, int first, float* A,
                             void* ws, size_t ws_bytes, hipStream_t st) {
  const size_t na = a_bytes(K);
  const int64_t Kp = quad_rows(K), qstep = Kp * 8 * 4;
  if (ws_bytes < na + (size_t)(XC_SLACK + quad_slack(K))) return FLR_ERR_WORKSPACE;
  const int64_t cap = (int64_t)((ws_bytes - na - XC_SLACK - quad_slack(K)) / (size_t)qstep) / XC_GROUP * XC_GROUP;
  if (cap < XC_GROUP) return FLR_ERR_WORKSPACE;
  const int64_t nseg = (R + cap - 1) / cap;
  const int64_t Rs = round_up_group((R + nseg - 1) / nseg);  // <= cap
  float* Xq = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + na);
  for (int64_t seg = 0; seg < nseg; ++seg) {
    const int64_t r0 = seg * Rs, steps = (R - r0 < Rs) ? R - r0 : Rs;
    if (steps <= 0) break;
    const int64_t NB = round_up_group(steps) / 4;
    int rc = launch_quad_transpose(X, ldx, K, r0, steps, NB, Kp, Xq, st);
    if (rc != FLR_OK) return rc;
    const int fst = (first && seg == 0) ? 1 : 0;
    if (form == Form::QuadWgLds || form == Form::QuadWgSgpr)
      rc = launch_ref_chain_w(form == Form::QuadWgLds, Xq, NB, Kp, K, fst, A, st);
    else
      rc = launch_ref_chain_s(form == Form::QuadWave8 ? 8 : 4, Xq, NB, Kp, K, fst, A, st);
    if (rc != FLR_OK) return rc;
  }
  return FLR_OK;
}

// The DPP forms: per segment the chain-major transpose (skipping the tap-major
// blocks), the tap blocks' rewrite, the chain kernel over tiles [t0, t1).
// Form::DeadRegions (every tile in one call) splits a segment into regions,
// each its own chain launch continuing A: a 3 x 3 block
// with a mask of DM_ONE / DM_FOUR that lies whole inside the segment at
// off % 8 == 0 is a dead region (its live taps rewritten compactly, its dead
// ones read from the shared dead stream), the stretches between them run as
// before.  Any other block is expanded from gdead as before: the same bits.
// *dflag: the device flag "a dead value of g is not finite", when a region ran.
static int run_chain_regions(Form form, const float* X, int64_t K, int64_t R, int64_t ldx,
                             const std::vector<TapBlock>& taps, const uint64_t* dead, const float* gdead, int64_t nneg,
                             int first, float* A, void* ws, size_t ws_bytes, int t0, int t1, hipStream_t st,
                             const int** dflag) {
  const size_t na = a_bytes(K);
  const int64_t per_step = K * 8 * 4;
  const int nn = (int)std::min<int64_t>(nneg, K);
  // the blocks that may run as dead regions, and their dead streams at the
  // workspace's end (then a flag word)
  std::vector<DeadBlock> db(taps.size());
  size_t tfloats = 0;
  if (form == Form::DeadRegions)
    for (size_t b = 0; b < taps.size(); ++b) {
      db[b] = dead_block(taps[b], dead[b]);
      if (!db[b].fast) continue;
      db[b].toff = (int64_t)tfloats;
      tfloats += (size_t)(8 * db[b].ldt);
    }
  size_t xc_end = ws_bytes;  // the chain-major streams end here
  if (tfloats > 0) {
    const size_t tb = tfloats * 4 + 256;
    if (ws_bytes >= na + (size_t)XC_SLACK + (size_t)(per_step * XC_GROUP) + tb + 256)
      xc_end = (ws_bytes - tb) / 256 * 256;
    else  // no room for the dead streams: every block expanded
      for (auto& b : db) b.fast = false;
  }
  float* Tall = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + xc_end);
  int* flag = reinterpret_cast<int*>(Tall + tfloats);
  const int64_t ldc = (int64_t)((xc_end - na - XC_SLACK) / (size_t)per_step) / XC_GROUP * XC_GROUP;
  if (ldc < XC_GROUP) return FLR_ERR_WORKSPACE;
  std::vector<Region> regs;
  // one segment when the regions of the whole chain fit (the dead regions are
  // shorter than their blocks), else segments of equal steps as before
  int64_t nseg = (R + ldc - 1) / ldc;
  if (tfloats > 0 && plan_regions(db, 0, R, true, regs) <= ldc) nseg = 1;
  const int64_t Rs = nseg == 1 ? R : round_up_group((R + nseg - 1) / nseg);  // <= ldc
  float* Xc0 = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + na);
  bool streams_made = false, started = false;
  for (int64_t seg = 0; seg < nseg; ++seg) {
    const int64_t sr0 = seg * Rs, ssteps = (R - sr0 < Rs) ? R - sr0 : Rs;
    if (ssteps <= 0) break;
    if (plan_regions(db, sr0, ssteps, tfloats > 0, regs) > ldc)
      plan_regions(db, sr0, ssteps, false, regs);  // (the padding of many regions)
    for (const Region& rg : regs) {
      const int fst = (first && !started) ? 1 : 0;
      started = true;
      float* Xc = Xc0 + rg.pos;
      int rc = FLR_OK;
      if (rg.blk >= 0) {  // a dead region
        const DeadBlock& d = db[(size_t)rg.blk];
        if (!streams_made) {  // every block's dead stream, once per call
          streams_made = true;
          if (hipMemsetAsync(Tall, 0, tfloats * 4 + 4, st) != hipSuccess) return FLR_ERR_HIP;
          for (size_t b = 0; b < taps.size(); ++b)
            if (db[b].fast &&
                (rc = launch_dead_stream(gdead, taps[b], db[b].deadp, db[b].ldt, Tall + db[b].toff, flag, st)) != FLR_OK)
              return rc;
          if (dflag) *dflag = flag;
        }
        // the live stream's slots no step fills: the first period and, from the
        // shortest chain's last period on, the rest of the padded stream
        const int64_t zs = d.S / 9 * d.live.nl;
        if ((rc = launch_zero_slots(Xc, ldc, K, d.live.nl, zs, d.Lp, st)) != FLR_OK) return rc;
        if ((rc = launch_tap_chain_live(X, K, ldx, taps[(size_t)rg.blk], d.r0, d.S, ldc, Xc, (uint64_t)d.dm, nn, d.live,
                                        st)) != FLR_OK)
          return rc;
        if ((rc = launch_ref_chain_dead(d.dm, Xc, ldc, Tall + d.toff, d.ldt, K, nn, d.Ll, fst, A, st)) != FLR_OK)
          return rc;
        continue;
      }
      const int64_t r0 = rg.a, steps = rg.b - rg.a;
      if ((rc = launch_chain_transpose(X, K, ldx, r0, steps, ldc, Xc, wave_runs(taps, r0, steps), st)) != FLR_OK)
        return rc;
      for (size_t b = 0; b < taps.size(); ++b) {  // the tap-major blocks of this segment, rewritten
        if (taps[b].end() <= 8 * r0 || taps[b].off >= 8 * (r0 + steps)) continue;
        if ((rc = launch_tap_chain(X, K, ldx, taps[b], r0, steps, ldc, Xc, gdead, dead ? dead[b] : 0, nn, st)) != FLR_OK)
          return rc;
      }
      const int64_t padded = round_up_group(steps);  // <= Rs <= ldc
      if (padded > steps && (rc = launch_zero_slots(Xc, ldc, K, 0, steps, padded, st)) != FLR_OK) return rc;
      rc = form == Form::DppTwo ? launch_ref_chain2(Xc, ldc, K, steps, fst, A, st)  // every pair: the two-chain tiles
                                : launch_ref_chain(Xc, ldc, K, steps, t0, t1, fst, A, st);
      if (rc != FLR_OK) return rc;
    }
  }
  return FLR_OK;
}

// The chains of tiles [t0, t1) over R chain steps of X (coordinates
// 0 .. 8 R - 1 of each row), continuing the sums in A (first: from 0), in the
// form pick_form chooses.  dead (with gdead, nneg): the blocks' dead-tap masks.
static int run_chains(const float* X, int64_t K, int64_t R, int64_t ldx, const std::vector<TapBlock>& taps,
                      const uint64_t* dead, const float* gdead, int64_t nneg, int first, float* A, void* ws,
                      size_t ws_bytes, int t0, int t1, hipStream_t st, const int** dflag) {
  if (ws_bytes < a_bytes(K) + (size_t)XC_SLACK) return FLR_ERR_WORKSPACE;
  const bool all_tiles = t0 == 0 && t1 == ntiles_of((int)K);
  const Form form = pick_form(K, (int64_t)taps.size(), all_tiles, dead && gdead);
  if (is_quad(form)) return run_quad_segments(form, X, K, R, ldx, first, A, ws, ws_bytes, st);
  return run_chain_regions(form, X, K, R, ldx, taps, dead, gdead, nneg, first, A, ws, ws_bytes, t0, t1, st, dflag);
}

static int check_rows(const float* X, int64_t K, int64_t n, int64_t ldx) {
  // 16-B loads of the rows
  if (K > 1 && n >= 8 && (((reinterpret_cast<uintptr_t>(X) & 15) != 0) || (ldx % 4) != 0)) return FLR_ERR_ARG;
  return FLR_OK;
}

extern "C" int flr_pairwise_l2_reference_tap_dead(const float* X, int64_t K, int64_t P, int64_t ldx,
                                                  const int64_t* taps, int64_t ntaps, const uint64_t* dead,
                                                  const float* gdead, int64_t nneg, double* D, void* ws,
                                                  size_t ws_bytes, int64_t part, int64_t nparts, void* stream) {
  if (K < 1 || P < 0 || ldx < P || !D || (K > 1 && P > 0 && !X) || nparts < 1 || part < 0 || part >= nparts)
    return FLR_ERR_ARG;
  if (K > (1 << 15)) return FLR_ERR_UNSUPPORTED;
  if (ntaps < 0 || (ntaps > 0 && !taps) || nneg < 0) return FLR_ERR_ARG;
  // tap-major blocks: {off, Cout, Cin, KK}, inside [0, P), ascending, disjoint
  std::vector<TapBlock> blocks;
  if (!parse_taps(taps, ntaps, P, blocks)) return FLR_ERR_ARG;
  bool any_dead = false;
  for (size_t b = 0; dead && b < blocks.size(); ++b) {  // bit t names tap t < min(KK, 64)
    if (blocks[b].kk < 64 && (dead[b] >> blocks[b].kk) != 0) return FLR_ERR_ARG;
    any_dead |= dead[b] != 0;
  }
  if (any_dead && !gdead) return FLR_ERR_ARG;
  int rc = check_rows(X, K, P, ldx);
  if (rc != FLR_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t R = P / 8;
  if (K > 1 && R > 0 && (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) != 0)) return FLR_ERR_WORKSPACE;
  const int ntiles = K > 1 ? ntiles_of((int)K) : 0;
  const int t0 = (int)(part * ntiles / nparts), t1 = (int)((part + 1) * ntiles / nparts);
  float* A = reinterpret_cast<float*>(ws);
  const int* dflag = nullptr;  // set by a dead region's plan (run_chain_regions)
  if (K > 1 && R > 0 && t1 > t0 &&
      (rc = run_chains(X, K, R, ldx, blocks, any_dead ? dead : nullptr, gdead, nneg, 1, A, ws, ws_bytes, t0, t1, st,
                       &dflag)) != FLR_OK)
    return rc;
  // the tail coordinates' columns (identity outside the tap-major blocks); the
  // finish kernel reads them from X, so none of them may be a dead tap
  TailCols tc;
  for (int64_t u = 8 * R; u < 8 * R + 8; ++u) {
    tc.c[u - 8 * R] = u;
    for (size_t b = 0; b < blocks.size() && u < P; ++b) {
      if (!blocks[b].contains(u)) continue;
      tc.c[u - 8 * R] = blocks[b].column_of(u);
      const int64_t t = blocks[b].tap_of(u);
      if (any_dead && t < 64 && ((dead[b] >> t) & 1)) return FLR_ERR_ARG;
    }
  }
  const int64_t kk = K * K;
  hipLaunchKernelGGL(ref_finish_kernel, dim3((unsigned)((kk + 255) / 256)), dim3(256), 0, st, A, R > 0 ? 1 : 0, X, tc,
                     (int)K, P, ldx, R, t0, t1, D, dflag, (int)std::min<int64_t>(nneg, K));
  return launch_status("ref_finish_kernel");
}

extern "C" int flr_pairwise_l2_reference_tap(const float* X, int64_t K, int64_t P, int64_t ldx,
                                             const int64_t* taps, int64_t ntaps, double* D, void* ws, size_t ws_bytes,
                                             int64_t part, int64_t nparts, void* stream) {
  return flr_pairwise_l2_reference_tap_dead(X, K, P, ldx, taps, ntaps, nullptr, nullptr, 0, D, ws, ws_bytes, part,
                                            nparts, stream);
}

extern "C" int flr_pairwise_l2_reference(const float* X, int64_t K, int64_t P, int64_t ldx, double* D, void* ws,
                                         size_t ws_bytes, int64_t part, int64_t nparts, void* stream) {
  return flr_pairwise_l2_reference_tap(X, K, P, ldx, nullptr, 0, D, ws, ws_bytes, part, nparts, stream);
}

extern "C" int flr_pairwise_l2_reference_partial_tap(const float* X, int64_t K, int64_t steps, int64_t ldx,
                                                     const int64_t* taps, int64_t ntaps, int first, void* ws,
                                                     size_t ws_bytes, void* stream) {
  if (K < 1 || steps < 0 || ldx < 8 * steps || (K > 1 && steps > 0 && !X)) return FLR_ERR_ARG;
  if (ntaps < 0 || (ntaps > 0 && !taps)) return FLR_ERR_ARG;
  // ascending, disjoint, wholly inside the slice's chain steps
  std::vector<TapBlock> blocks;
  if (!parse_taps(taps, ntaps, 8 * steps, blocks)) return FLR_ERR_ARG;
  if (K > (1 << 15)) return FLR_ERR_UNSUPPORTED;
  int rc = check_rows(X, K, 8 * steps, ldx);
  if (rc != FLR_OK) return rc;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) != 0 || ws_bytes < a_bytes(K)) return FLR_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  float* A = reinterpret_cast<float*>(ws);
  if (K < 2) return FLR_OK;
  if (steps == 0) {  // nothing to add; a first call still starts every chain at 0
    if (first && hipMemsetAsync(A, 0, (size_t)8 * K * K * 4, st) != hipSuccess)
      return launch_status("reference distances: zero the chains");
    return FLR_OK;
  }
  return run_chains(X, K, steps, ldx, blocks, nullptr, nullptr, 0, first, A, ws, ws_bytes, 0, ntiles_of((int)K), st,
                    nullptr);
}

extern "C" int flr_pairwise_l2_reference_partial(const float* X, int64_t K, int64_t steps, int64_t ldx, int first,
                                                 void* ws, size_t ws_bytes, void* stream) {
  return flr_pairwise_l2_reference_partial_tap(X, K, steps, ldx, nullptr, 0, first, ws, ws_bytes, stream);
}

extern "C" int flr_pairwise_l2_reference_finish(const float* Xtail, int64_t K, int64_t ntail, int64_t ldx,
                                                int chains, const void* ws, double* D, void* stream) {
  if (K < 1 || ntail < 0 || ntail > 7 || ldx < ntail || !D || (K > 1 && ntail > 0 && !Xtail) ||
      (K > 1 && chains && !ws))
    return FLR_ERR_ARG;
  if (K > (1 << 15)) return FLR_ERR_UNSUPPORTED;
  TailCols tc;
  for (int u = 0; u < 8; ++u) tc.c[u] = u;
  const int64_t kk = K * K;
  hipLaunchKernelGGL(ref_finish_kernel, dim3((unsigned)((kk + 255) / 256)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const float*>(ws), chains ? 1 : 0, Xtail, tc, (int)K, ntail, ldx, (int64_t)0, 0,
                     K > 1 ? ntiles_of((int)K) : 0, D, nullptr, 0);
  return launch_status("ref_finish_kernel");
}
