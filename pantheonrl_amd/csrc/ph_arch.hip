// MLP towers of a run-time shape: SB3's MlpPolicy with policy_kwargs net_arch = [dict(pi = W, vf = W)], W one to three widths
// that are multiples of 32 up to 256 (the extractor loop is reference pantheonrl/algos/adap/policies.py:152-200: Linear then
// Tanh for every listed width).  Forward (tower_fwd_kernel) and PPO minibatch gradient (tower_grad_kernel), beside the 64-wide
// kernels, never inside them: PH_HIDDEN and everything built on it stay as they are.
//
// Both kernels: grid (workgroups, 2), blockIdx.y = policy / value net, 256 lanes, R rows per tile.  Every layer's activations of
// the tile stay in LDS ([R][w_l + 1]: the odd leading dimension keeps the transposed-operand reads conflict free); weights stream
// through ONE staged block of LDS, 64 x NBW going forward and NBW x 64 going back (NBW = 64 at R = 64, 128 at R = 32: four 32x32
// output tiles per staged block, one per wave).  All products are tile_mma (v_mfma_f32_32x32x2_f32, or its VALU restatement with
// the same accumulation order: gemm_mode 1 gives the bits of mode 0).  Weight gradients accumulate in the workgroup's slab of P
// floats in parameter order, so the reduce / clip / Adam launches of the 64-wide path take them unchanged.
#include "ph_rowtail.h"
#include "ph_arch.h"
#include "ph_ppo_loss.h"
#include "ph_pool.h"

namespace ph {

namespace {

constexpr int TNT = 256;   // lanes of a workgroup

// s + sum_{r < N} p[r * stride] in row order, 16 LDS reads in flight at a time
template <int N>
__device__ __forceinline__ float tw_colsum(const float* p, int stride, float s) {
#pragma unroll
  for (int r0 = 0; r0 < N; r0 += 16) {
    float t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = p[(r0 + i) * stride];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) s += t[i];
  }
  return s;
}
template <int N>
__device__ __forceinline__ float tw_coldot(const float* p, int stride, const float* q, float s) {
#pragma unroll
  for (int r0 = 0; r0 < N; r0 += 16) {
    float t[16], u[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      t[i] = p[(r0 + i) * stride];
      u[i] = q[r0 + i];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) s = __builtin_fmaf(t[i], u[i], s);
  }
  return s;
}

// dst[r][c] (leading dimension ldd) = W[(r0 + r) * ldw + c0 + c] for r < NR, c < NC; zero where r0 + r >= nrows or c0 + c >= ncols.
// ldw, c0 and ncols are multiples of 4 and W is 16-byte aligned (tower weights: every offset of the layout up to act_W is a
// multiple of 32 floats): 16-byte global loads, all of a lane's loads in flight before the first LDS store.
template <int NR, int NC>
__device__ __forceinline__ void stage_block(float* dst, int ldd, const float* W, int ldw, int r0, int nrows, int c0, int ncols, int tid) {
  constexpr int ITERS = NR * NC / 4 / TNT;
  float4 v[ITERS];
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int q = tid + TNT * i;
    const int r = q / (NC / 4), c = (q - r * (NC / 4)) * 4;
    const bool ok = (r0 + r < nrows) && (c0 + c < ncols);
    v[i] = ok ? *reinterpret_cast<const float4*>(W + (size_t)(r0 + r) * ldw + c0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < ITERS; ++i) {
    const int q = tid + TNT * i;
    const int r = q / (NC / 4), c = (q - r * (NC / 4)) * 4;
    float* d = dst + r * ldd + c;
    d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
  }
}
// rows [r0, r0 + nr) of act_W[nrows][L] -> dst[nr][ldo], columns [L, Lp) and rows >= nrows zero (L is arbitrary: 4-byte loads,
// eight in flight per lane)
__device__ __forceinline__ void stage_head(float* dst, int ldo, const float* Wo, int L, int Lp, int r0, int nr, int nrows, int tid) {
  const int total = nr * Lp;
  for (int e0 = 0; e0 < total; e0 += 8 * TNT) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = e0 + tid + TNT * i;
      const int r = e / Lp, c = e - r * Lp;
      v[i] = (e < total && r0 + r < nrows && c < L) ? Wo[(size_t)(r0 + r) * L + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = e0 + tid + TNT * i;
      const int r = e / Lp, c = e - r * Lp;
      if (e < total) dst[r * ldo + c] = v[i];
    }
  }
}

// X chunk c of the tile -> bufx [R][LDH].  Caller: bufx free (barrier before), barrier after.
template <int R>
__device__ __forceinline__ void stage_x(XStage<R, TNT>& xr, float* bufx, const int* rowphys, const float* obs, const NetDims& nd,
                                        const int* fcomp, int c, int tid) {
  if (nd.obs_kind == PH_SPACE_BOX) {
    xr.issue(rowphys, obs, nd, c, tid);
    xr.commit(bufx, rowphys, obs, nd, c, tid);
  } else {
    xr.commit_onehot(bufx, fcomp, nd, c, tid);
  }
}

// biases of this net's layers and the head vector (act_b | val_W) -> LDS; caller barriers afterwards
__device__ __forceinline__ void stage_biases(float* smem, const ArchLds& S, const float* params, const ArchDims& ad, const NetDims& nd,
                                             int net, int tid) {
  const int wn = pick3(ad.w, ad.nl - 1);
  for (int l = 0; l < ad.nl; ++l) {
    const int w = pick3(ad.w, l), ob = net == 0 ? pick3(ad.lay.pi_b, l) : pick3(ad.lay.vf_b, l);
    if (tid < w) smem[S.bias + l * PH_ARCH_MAX_WIDTH + tid] = params[ob + tid];
  }
  if (net == 0) smem[S.bos + tid] = tid < nd.L ? params[ad.lay.act_b + tid] : 0.f;
  else smem[S.bos + tid] = tid < wn ? params[ad.lay.val_W + tid] : 0.f;
}

// Both towers' forward pass of one tile: H_l = tanh(H_{l-1} W_l + b_l) into S.act[l], layer by layer, weights streamed.
// Ends with a barrier: every activation of the tile is visible.
template <int R, bool VALU>
__device__ __forceinline__ void towers_forward(float* smem, const ArchLds& S, const float* params, const ArchDims& ad, const NetDims& nd,
                                               int net, const float* obs, const int* rowphys, XStage<R, TNT>& xr, const int* fcomp,
                                               int tid) {
  constexpr int MT = R / 32, NTB = 4 / MT, NBW = 32 * NTB;
  const int wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int mt = wave / NTB, nt = wave - mt * NTB;
  float* bufx = smem + S.bufx;
  float* wst = smem + S.wst;
  for (int l = 0; l < ad.nl; ++l) {
    const int N = pick3(ad.w, l);
    const int K = l == 0 ? nd.nchunk * HID : pick3(ad.w, l - 1);
    const int krows = l == 0 ? nd.F : K;   // rows W_l really has
    const float* Wg = params + (net == 0 ? pick3(ad.lay.pi_W, l) : pick3(ad.lay.vf_W, l));
    const float* A = l == 0 ? bufx : smem + pick3(S.act, l - 1);
    const int lda = l == 0 ? LDH : K + 1;
    float* out = smem + pick3(S.act, l);
    const int ldo = N + 1;
    const float* bias = smem + S.bias + l * PH_ARCH_MAX_WIDTH;
    for (int n0 = 0; n0 < N; n0 += NBW) {
      const int col = n0 + nt * 32;
      f32x16 acc = {0};
      for (int k0 = 0; k0 < K; k0 += HID) {
        __syncthreads();   // the staged block (and X chunk) consumed; the layer below complete
        if (l == 0) stage_x<R>(xr, bufx, rowphys, obs, nd, fcomp, k0 / HID, tid);
        stage_block<HID, NBW>(wst, NBW + 1, Wg, N, k0, krows, n0, N, tid);
        __syncthreads();
        const int klen = K - k0 < HID ? K - k0 : HID;
        if (col < N)
          acc = tile_mma<false, false, VALU>(l == 0 ? A : A + k0, lda, wst, NBW + 1, mt * 32, nt * 32, 0, klen, acc, lane);
      }
      if (col < N) {
        const float bb = bias[col + li];
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(mt * 32 + drow(r, lh)) * ldo + col + li] = fast_tanh(acc[r] + bb);
      }
    }
  }
  __syncthreads();
}

// logits = H_n act_W + act_b -> outs [R][Lp + 1]; act_W streams in 64-row blocks.  Ends with a barrier.
template <int R, bool VALU>
__device__ __forceinline__ void head_logits(float* smem, const ArchLds& S, const float* params, const ArchDims& ad, const NetDims& nd,
                                            int tid) {
  constexpr int MT = R / 32;
  const int wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  const int Lp = nd.Lp, LDO = Lp + 1, ntn = Lp >> 5;
  const int wn = pick3(ad.w, ad.nl - 1), ldh = wn + 1;
  const float* Hn = smem + pick3(S.act, ad.nl - 1);
  float* wst = smem + S.wst;
  float* outs = smem + S.bufx;
  const bool on = wave < MT * ntn;
  const int hm = wave / ntn, hn = wave - hm * ntn;
  f32x16 acc = {0};
  for (int k0 = 0; k0 < wn; k0 += HID) {
    __syncthreads();
    stage_head(wst, LDO, params + ad.lay.act_W, nd.L, Lp, k0, HID, wn, tid);
    __syncthreads();
    const int klen = wn - k0 < HID ? wn - k0 : HID;
    if (on) acc = tile_mma<false, false, VALU>(Hn + k0, ldh, wst, LDO, hm * 32, hn * 32, 0, klen, acc, lane);
  }
  if (on) {
    const float bb = smem[S.bos + hn * 32 + li];
#pragma unroll
    for (int r = 0; r < 16; ++r) outs[(hm * 32 + drow(r, lh)) * LDO + hn * 32 + li] = acc[r] + bb;
  }
  __syncthreads();
}

}  // namespace

// ---- forward ---------------------------------------------------------------------------------------------------------------
// What a forward workgroup stages once: its tile's row indices (relative to a.obs), this net's biases and head vector, the
// one-hot feature -> component table.  Caller barriers afterwards.  `map` (the pool's grouped forward): the tile's rows are the
// tables map[0 .. rows) instead of row0 .. row0 + 31.
__device__ __forceinline__ void tower_fwd_setup(float* smem, const ArchLds& S, const FwdArgs& a, const ArchDims& ad, int net, int row0,
                                                int tid, const int* map = nullptr, int rows = 0) {
  constexpr int R = ARCH_FWD_ROWS;
  int* rowphys = (int*)(smem + S.rowphys);
  if (tid < R) {
    if (map) rowphys[tid] = tid < rows ? map[tid] : -1;
    else rowphys[tid] = (row0 + tid < a.n) ? row0 + tid : -1;
  }
  stage_biases(smem, S, a.params, ad, a.nd, net, tid);
  if (a.nd.obs_kind != PH_SPACE_BOX) XStage<R, TNT>::build_fcomp((int*)(smem + S.fcomp), a.nd, tid);
}

// One forward of the workgroup's tile after tower_fwd_setup (and a barrier): every layer's products, then the value net's row
// tail and observation copy, or the head product and the sampling tail.  Every global store goes through value_row_tail /
// copy_obs_rows / general_row_tail, i.e. through rb_row: rectangular and ragged rollout-buffer rows alike.
// MAP (the pool's grouped forward): the tile's rows are the tables rowphys[0 .. rows), in any order -- every tail and the
// observation copy address table rowphys[t] instead of row0 + t.  The products are the same either way: they read rowphys only.
template <bool VALU, bool MAP = false>
__device__ __forceinline__ void tower_fwd_body(float* smem, const ArchLds& S, const FwdArgs& a, const ArchDims& ad, int net, int row0,
                                               int tid, int rows = 0) {
  constexpr int R = ARCH_FWD_ROWS;
  const NetDims& nd = a.nd;
  const bool onehot = nd.obs_kind != PH_SPACE_BOX;
  int* rowphys = (int*)(smem + S.rowphys);
  int* feat = (int*)(smem + S.feat);
  int* fcomp = (int*)(smem + S.fcomp);
  XStage<R, TNT> xr;
  if (onehot) xr.build_feat(feat, rowphys, a.obs, nd, tid);
  towers_forward<R, VALU>(smem, S, a.params, ad, nd, net, a.obs, rowphys, xr, fcomp, tid);
  const int wn = pick3(ad.w, ad.nl - 1), ldh = wn + 1;
  const float* Hn = smem + pick3(S.act, ad.nl - 1);
  if (net == 1) {
    if (tid < R && rowphys[tid] >= 0) {
      float v = 0.f;
      for (int j = 0; j < wn; ++j) v = __builtin_fmaf(Hn[tid * ldh + j], smem[S.bos + j], v);
      value_row_tail(a, MAP ? rowphys[tid] : row0 + tid, v + a.params[ad.lay.val_b]);
    }
    if constexpr (MAP) {
      if (a.rb_obs)
        for (int e = tid; e < rows * nd.D; e += TNT) {
          const int r = e / nd.D, d = e - r * nd.D, gt = rowphys[r];
          const long long ridx = rb_row(a, gt);
          if (ridx >= 0) a.rb_obs[(size_t)ridx * nd.D + d] = a.obs[(size_t)gt * nd.D + d];
        }
    } else {
      copy_obs_rows(a, row0, (a.n - row0 < R) ? a.n - row0 : R, nd.D);
    }
    return;
  }
  head_logits<R, VALU>(smem, S, a.params, ad, nd, tid);
  if (tid < R && rowphys[tid] >= 0)
    general_row_tail(a, nd, MAP ? rowphys[tid] : row0 + tid, smem + S.bufx + tid * (nd.Lp + 1), fwd_counter(a));
}

template <bool VALU>
__global__ __launch_bounds__(TNT) void tower_fwd_kernel(FwdArgs a, ArchDims ad) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = ARCH_FWD_ROWS;
  const bool onehot = a.nd.obs_kind != PH_SPACE_BOX;
  const ArchLds S = arch_lds(ad, R, onehot ? a.nd.D : 0, a.nd.nchunk);
  const int tid = threadIdx.x, net = blockIdx.y, row0 = blockIdx.x * R;
  tower_fwd_setup(smem, S, a, ad, net, row0, tid);
  __syncthreads();
  tower_fwd_body<VALU>(smem, S, a, ad, net, row0, tid);
}

// ---- the tower tiles of the pool's grouped forward (ph_pool.h) ----------------------------------------------------------------------
// One workgroup per (tile of the bucket pass, net), as pool_fwd16h_kernel: the tile names a member and <= 16 sorted positions.  A
// tile whose member is no tower is another kernel's.  The member's part (weights, seed, caches, ragged buffer) is patched into the
// workgroup's copy of the shared record exactly as pool_fwd16h_kernel does, and the member's ArchDims come from the member table in
// DEVICE memory (uniform loads; a by-value array of them indexed by the member would send the argument block to scratch, ph_arch.h).
// The forward is the 32-row body, half empty: rowphys[t] = order[first + t] for t < rows, else -1, so a table's products, tails and
// draws -- (member seed, counter, table) -- are those of ph_arch_forward over all tables, bit for bit.  The launch's dynamic LDS is the
// largest carve over the table's tower members; a workgroup carves with its own member's arch_lds.
template <bool VALU>
__global__ __launch_bounds__(TNT) void pool_tower_kernel(PoolFwd p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = ARCH_FWD_ROWS;
  const int tile = blockIdx.x;
  if (tile >= p.b.ntiles[0]) return;
  const int member = p.b.tiles[3 * tile], first = p.b.tiles[3 * tile + 1];
  const int rows = p.b.tiles[3 * tile + 2] < POOL_TILE ? p.b.tiles[3 * tile + 2] : POOL_TILE;   // (device data: clamped once)
  const PoolMemberDev& m = p.members[member];
  if (!m.tower) return;   // pool_fwd16h_kernel's or pool_clone16_kernel's
  const bool learner = m.kind == PH_POOL_LEARNER;
  const int tid = threadIdx.x, net = blockIdx.y;
  if (net == 1 && !learner && !m.values) return;
  const ArchDims ad = m.ad;
  FwdArgs a = p.a;
  a.params = m.params;
  a.seed = m.seed;
  a.values = m.values;
  a.logp = m.log_probs;
  if (learner) {
    a.rb_obs = m.rb_obs;
    a.rb_act = m.rb_act;
    a.rb_rew = m.rb_rew;
    a.rb_es = m.rb_es;
    a.rb_val = m.rb_val;
    a.rb_logp = m.rb_logp;
    a.pos_env = m.pos;
    a.rb_T = m.rb_T;
  } else {
    a.pos_env = nullptr;
    a.rec_mask = nullptr;
    a.es_in = nullptr;
  }
  const bool onehot = a.nd.obs_kind != PH_SPACE_BOX;
  const ArchLds S = arch_lds(ad, R, onehot ? a.nd.D : 0, a.nd.nchunk);
  tower_fwd_setup(smem, S, a, ad, net, 0, tid, p.b.order + first, rows);
  __syncthreads();
  tower_fwd_body<VALU, true>(smem, S, a, ad, net, 0, tid, rows);
}

// ---- one-launch rollout against a scripted environment ---------------------------------------------------------------------------
// sc.n_steps forwards of the same tile in one launch (the contract of ph_scripted_rollout, for towers): a workgroup owns its 32
// rows of one net for the whole rollout, stages biases / head vector / fcomp once and loops tower_fwd_body, advancing the step's
// argument record in registers -- observation row block t, rollout-buffer rows pos0 + t, episode starts and the late reward of
// step t - 1, Philox counter counter0 + t.  A row's scalars are written by the same lane in every step and rows are independent:
// no workgroup ever waits for another one.  Weights stream through LDS per step, as in the single forward.
template <bool VALU>
__global__ __launch_bounds__(TNT) void tower_rollout_kernel(FwdArgs a, ArchDims ad, ScriptedSteps sc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = ARCH_FWD_ROWS;
  const bool onehot = a.nd.obs_kind != PH_SPACE_BOX;
  const ArchLds S = arch_lds(ad, R, onehot ? a.nd.D : 0, a.nd.nchunk);
  const int tid = threadIdx.x, net = blockIdx.y, row0 = blockIdx.x * R;
  tower_fwd_setup(smem, S, a, ad, net, row0, tid);
  const size_t n = (size_t)a.n, nD = n * a.nd.D, nA = n * a.nd.A;
  FwdArgs s = a;   // step t's record
  for (int t = 0; t < sc.n_steps; ++t) {
    __syncthreads();   // first pass: the staged vectors are visible; later: the previous step's tails are done with LDS
    tower_fwd_body<VALU>(smem, S, s, ad, net, row0, tid);
    s.obs += nD;
    s.rb_obs += nD;
    s.rb_act += nA;
    s.prev_rew = s.rb_rew;
    s.rb_rew += n;
    s.rb_es += n;
    s.rb_val += n;
    s.rb_logp += n;
    s.es_in = sc.done_seq + (size_t)t * n;
    s.pending_reward = sc.rew_seq + (size_t)t * n;
    s.counter += 1;
  }
  // the last step's reward: added to the 0 this lane stored in that row (ph_buffer_add_reward's arithmetic: 0 + (-0) is +0)
  if (net == 1 && tid < R && row0 + tid < a.n) s.prev_rew[row0 + tid] += s.pending_reward[row0 + tid];
}

// ---- PPO minibatch gradient ----------------------------------------------------------------------------------------------------
// Per tile: forward keeping every layer's activations, loss and head gradient, then per layer from the top dZ = dH (1 - H^2) (in
// place over H), dW += in^T dZ, db += colsum dZ, dH_below = dZ W^T (not below layer 1).  Rows are gathered through the minibatch
// order exactly as ppo_grad_kernel does (minibatch_row).
template <int R, bool VALU>
__global__ __launch_bounds__(TNT) void tower_grad_kernel(GradArgs a, ArchDims ad) {
  if (*a.stop_flag) return;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int MT = R / 32, NTB = 4 / MT, NBW = 32 * NTB;
  const NetDims& nd = a.nd;
  const bool onehot = nd.obs_kind != PH_SPACE_BOX;
  const ArchLds S = arch_lds(ad, R, onehot ? nd.D : 0, nd.nchunk);
  float* bufx = smem + S.bufx;
  float* outs = bufx;
  float* wst = smem + S.wst;
  float* bos = smem + S.bos;
  float* radv = smem + S.radv;
  float* rold = smem + S.rold;
  float* rdv = smem + S.rdv;
  float* red = smem + S.red;
  int* rowphys = (int*)(smem + S.rowphys);
  int* feat = (int*)(smem + S.feat);
  int* fcomp = (int*)(smem + S.fcomp);
  const int tid0 = threadIdx.x, net = blockIdx.y;
  const int Lp = nd.Lp, LDO = Lp + 1, ntn = Lp >> 5;
  const int wn = pick3(ad.w, ad.nl - 1), ldh = wn + 1;
  float* Hn = smem + pick3(S.act, ad.nl - 1);
  float* slab = a.slabs + (size_t)blockIdx.x * ad.lay.P;
  const float inv_nb = 1.0f / (float)a.nb;

  float st[NSTATP];
#pragma unroll
  for (int k = 0; k < NSTATP; ++k) st[k] = 0.f;

  // row metadata of one tile (gather indices -> physical rows, per-row scalars)
  auto stage_rows = [&](int tile) {
    if (tid0 < R) {
      const int gi = tile * R + tid0;
      int phys = -1;
      float adv = 0.f, old = 0.f;
      if (gi < a.nb) {
        phys = minibatch_row(a, gi);
        if (net == 0) {
          adv = a.rb_adv[phys];
          if (a.norm_adv && a.nb > 1) adv = (adv - a.advstats[0]) / (a.advstats[1] + 1e-8f);
          old = a.rb_logp[phys];
        } else {
          adv = a.rb_ret[phys];
          old = a.rb_val[phys];
        }
      }
      rowphys[tid0] = phys;
      radv[tid0] = adv;
      rold[tid0] = old;
    }
  };
  stage_rows(blockIdx.x);
  stage_biases(smem, S, a.params, ad, nd, net, tid0);
  if (onehot) XStage<R, TNT>::build_fcomp(fcomp, nd, tid0);

  bool first = true;
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x, first = false) {
    __syncthreads();  // row metadata (and, first time, biases / fcomp) visible
    // thread-id-derived coordinates are re-materialised per tile from an opaque copy of threadIdx.x, or the compiler hoists the
    // per-register LDS / slab addresses of every phase out of the tile loop and pins them in VGPRs (as in ppo_grad_kernel)
    int tidv = threadIdx.x;
    asm volatile("" : "+v"(tidv));
    const int tid = tidv, lane = tid & 63, wave = tid >> 6;
    const int mt = wave / NTB, nt = wave - mt * NTB;
    const int li = lane & 31, lh = lane >> 5;

    XStage<R, TNT> xr;
    if (onehot) xr.build_feat(feat, rowphys, a.rb_obs, nd, tid);
    towers_forward<R, VALU>(smem, S, a.params, ad, nd, net, a.rb_obs, rowphys, xr, fcomp, tid);

    if (net == 0) {
      head_logits<R, VALU>(smem, S, a.params, ad, nd, tid);
      if (tid < R) {   // one lane per row: dL/dlogits over the row's logits, partial statistics into st
        float* z = outs + tid * LDO;
        const int phys = rowphys[tid];
        if (phys < 0) {
          for (int k = 0; k < Lp; ++k) z[k] = 0.f;
        } else {
          ppo_two_pass_row(nd, z, a.rb_act, phys, radv[tid], rold[tid], a.clip, a.ent_coef, inv_nb, st, Lp);
        }
      }
      __syncthreads();
      // d act_W = H_n^T dOut (tiles w_n/32 x Lp/32), d act_b = column sums of dOut
      for (int t = wave; t < (wn >> 5) * ntn; t += 4) {
        const int hm = t / ntn, hn = t - hm * ntn;
        f32x16 g = {0};
        if (!first) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = hm * 32 + drow(r, lh), col = hn * 32 + li;
            if (col < nd.L) g[r] = slab[ad.lay.act_W + j * nd.L + col];
          }
        }
        g = tile_mma<true, false, VALU>(Hn, ldh, outs, LDO, hm * 32, hn * 32, 0, R, g, lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = hm * 32 + drow(r, lh), col = hn * 32 + li;
          if (col < nd.L) slab[ad.lay.act_W + j * nd.L + col] = g[r];
        }
      }
      if (tid >= TNT - 64 && tid - (TNT - 64) < nd.L) {
        const int k = tid - (TNT - 64);
        float s = first ? 0.f : slab[ad.lay.act_b + k];
        s = tw_colsum<R>(outs + k, LDO, s);
        slab[ad.lay.act_b + k] = s;
      }
      // dH_n = dOut act_W^T ; dZ_n = dH_n (1 - H_n^2) in place
      for (int n0 = 0; n0 < wn; n0 += NBW) {
        __syncthreads();   // staged block consumed; first pass: every wave is done reading H_n for d act_W
        stage_head(wst, LDO, a.params + ad.lay.act_W, nd.L, Lp, n0, NBW, wn, tid);
        __syncthreads();
        const int col = n0 + nt * 32;
        if (col < wn) {
          f32x16 d = {0};
          d = tile_mma<false, true, VALU>(outs, LDO, wst, LDO, mt * 32, nt * 32, 0, Lp, d, lane);
          float hv[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) hv[r] = Hn[(mt * 32 + drow(r, lh)) * ldh + col + li];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int r = 0; r < 16; ++r) Hn[(mt * 32 + drow(r, lh)) * ldh + col + li] = d[r] * (1.0f - hv[r] * hv[r]);
        }
      }
    } else {
      // value net: v = H_n . val_W + val_b ; value loss ; dv
      if (tid < R) {
        const int phys = rowphys[tid];
        float dv = 0.f;
        if (phys >= 0) {
          float v = 0.f;
          for (int j = 0; j < wn; ++j) v = __builtin_fmaf(Hn[tid * ldh + j], bos[j], v);
          v += a.params[ad.lay.val_b];
          const float retn = radv[tid], oldv = rold[tid];
          const ValueRow vr = ppo_value_row(v, oldv, retn, a.clip_vf, a.vf_coef, inv_nb);
          st[1] += vr.err * vr.err;
          dv = vr.dv();
        }
        rdv[tid] = dv;
      }
      __syncthreads();
      if (tid < wn) {   // d val_W[j] = sum_r H_n[r][j] dv[r]
        float s = first ? 0.f : slab[ad.lay.val_W + tid];
        s = tw_coldot<R>(Hn + tid, ldh, rdv, s);
        slab[ad.lay.val_W + tid] = s;
      }
      if (tid == TNT - 1) {
        float s = first ? 0.f : slab[ad.lay.val_b];
        s = tw_colsum<R>(rdv, 1, s);
        slab[ad.lay.val_b] = s;
      }
      __syncthreads();
      for (int e = tid; e < R * wn; e += TNT) {   // dZ_n[r][j] = dv[r] val_W[j] (1 - H_n^2) in place
        const int r = e / wn, j = e - r * wn;
        const float h = Hn[r * ldh + j];
        Hn[r * ldh + j] = rdv[r] * bos[j] * (1.0f - h * h);
      }
    }

    // ---- layers from the top: dZ_l sits in S.act[l] ----
    for (int l = ad.nl - 1; l >= 0; --l) {
      __syncthreads();   // dZ_l complete
      const int N = pick3(ad.w, l), ldz = N + 1, nn = N >> 5;
      const float* dZ = smem + pick3(S.act, l);
      const int oW = net == 0 ? pick3(ad.lay.pi_W, l) : pick3(ad.lay.vf_W, l);
      const int oB = net == 0 ? pick3(ad.lay.pi_b, l) : pick3(ad.lay.vf_b, l);
      if (tid < N) {
        float s = first ? 0.f : slab[oB + tid];
        s = tw_colsum<R>(dZ + tid, ldz, s);
        slab[oB + tid] = s;
      }
      if (l > 0) {
        const int Kin = pick3(ad.w, l - 1), ldi = Kin + 1;
        float* Hin = smem + pick3(S.act, l - 1);
        // dW_l = H_{l-1}^T dZ_l
        for (int t = wave; t < (Kin >> 5) * nn; t += 4) {
          const int km = t / nn, kn = t - km * nn;
          f32x16 g = {0};
          if (!first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = slab[oW + (km * 32 + drow(r, lh)) * N + kn * 32 + li];
          }
          g = tile_mma<true, false, VALU>(Hin, ldi, dZ, ldz, km * 32, kn * 32, 0, R, g, lane);
#pragma unroll
          for (int r = 0; r < 16; ++r) slab[oW + (km * 32 + drow(r, lh)) * N + kn * 32 + li] = g[r];
        }
        // dH_{l-1} = dZ_l W_l^T ; dZ_{l-1} = dH_{l-1} (1 - H_{l-1}^2) in place.  (The first barrier below also says every wave
        // is done reading H_{l-1} for dW_l.)
        const float* Wg = a.params + oW;
        for (int n0 = 0; n0 < Kin; n0 += NBW) {
          const int col = n0 + nt * 32;
          f32x16 d = {0};
          for (int k0 = 0; k0 < N; k0 += HID) {
            __syncthreads();
            stage_block<NBW, HID>(wst, HID + 1, Wg, N, n0, Kin, k0, N, tid);
            __syncthreads();
            const int klen = N - k0 < HID ? N - k0 : HID;
            if (col < Kin) d = tile_mma<false, true, VALU>(dZ + k0, ldz, wst, HID + 1, mt * 32, nt * 32, 0, klen, d, lane);
          }
          if (col < Kin) {
            float hv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) hv[r] = Hin[(mt * 32 + drow(r, lh)) * ldi + col + li];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) Hin[(mt * 32 + drow(r, lh)) * ldi + col + li] = d[r] * (1.0f - hv[r] * hv[r]);
          }
        }
      } else {
        // dW_1 = X^T dZ_1 per feature chunk (bufx is free again: the head phases are over)
        for (int c = 0; c < nd.nchunk; ++c) {
          __syncthreads();
          stage_x<R>(xr, bufx, rowphys, a.rb_obs, nd, fcomp, c, tid);
          __syncthreads();
          for (int t = wave; t < 2 * nn; t += 4) {
            const int km = t / nn, kn = t - km * nn;
            f32x16 g = {0};
            if (!first) {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int k = c * HID + km * 32 + drow(r, lh);
                if (k < nd.F) g[r] = slab[oW + (size_t)k * N + kn * 32 + li];
              }
            }
            g = tile_mma<true, false, VALU>(bufx, LDH, dZ, ldz, km * 32, kn * 32, 0, R, g, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int k = c * HID + km * 32 + drow(r, lh);
              if (k < nd.F) slab[oW + (size_t)k * N + kn * 32 + li] = g[r];
            }
          }
        }
      }
    }
    if (tile + (int)gridDim.x < a.ntiles) {
      __syncthreads();  // this tile's row metadata fully consumed
      stage_rows(tile + gridDim.x);
    }
  }

  // ---- per-workgroup partial statistics (fixed reduction tree -> deterministic) ----
  const int lane0 = tid0 & 63, wave0 = tid0 >> 6;
#pragma unroll
  for (int k = 0; k < NSTATP; ++k) {
    float v = st[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    st[k] = v;
  }
  __syncthreads();
  if (lane0 == 0) {
#pragma unroll
    for (int k = 0; k < NSTATP; ++k) red[wave0 * NSTATP + k] = st[k];
  }
  __syncthreads();
  if (tid0 < NSTATP) {
    float v = 0.f;
    for (int w = 0; w < 4; ++w) v += red[w * NSTATP + tid0];
    a.statpart[((size_t)net * gridDim.x + blockIdx.x) * NSTATP + tid0] = v;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
size_t arch_grad_lds_bytes(const NetDims& nd, const ArchDims& ad, int R) {
  return sizeof(float) * (size_t)arch_lds(ad, R, nd.obs_kind != PH_SPACE_BOX ? nd.D : 0, nd.nchunk).total;
}
int arch_grad_rows(const NetDims& nd, const ArchDims& ad) { return arch_grad_lds_bytes(nd, ad, 64) <= ARCH_LDS_MAX ? 64 : 32; }
size_t arch_fwd_lds_bytes(const NetDims& nd, const ArchDims& ad) { return arch_grad_lds_bytes(nd, ad, ARCH_FWD_ROWS); }

void arch_grad_plan(const NetDims& nd, const ArchDims& ad, int nb, int num_cu, int* ntiles, int* nwg) {
  const int R = arch_grad_rows(nd, ad);
  *ntiles = (nb + R - 1) / R;
  // two nets x nwg workgroups; a carve above half the CU's LDS keeps one workgroup per CU resident
  int cap = arch_grad_lds_bytes(nd, ad, R) > ARCH_LDS_MAX / 2 ? num_cu / 2 : num_cu;
  const size_t by_slabs = ARCH_SLAB_CAP_BYTES / (sizeof(float) * (size_t)ad.lay.P);
  if ((size_t)cap > by_slabs) cap = (int)by_slabs;
  if (cap < 1) cap = 1;
  *nwg = *ntiles < cap ? *ntiles : cap;
}

template <int R, bool VALU>
static hipError_t launch_grad_inst(const GradArgs& a, const ArchDims& ad, int nwg, size_t lds, hipStream_t s) {
  if (const hipError_t e = allow_dynamic_lds((const void*)tower_grad_kernel<R, VALU>, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((tower_grad_kernel<R, VALU>), dim3(nwg, 2), dim3(TNT), lds, s, a, ad);
  return hipGetLastError();
}

hipError_t launch_arch_grad(const GradArgs& a, const ArchDims& ad, int nwg, int gemm_mode, hipStream_t s) {
  if (a.nd.gauss || (a.nd.Lp != 32 && a.nd.Lp != 64) || nwg < 1) return hipErrorInvalidValue;
  const int R = arch_grad_rows(a.nd, ad);
  const size_t lds = arch_grad_lds_bytes(a.nd, ad, R);
  if (lds > ARCH_LDS_MAX || a.ntiles != (a.nb + R - 1) / R) return hipErrorInvalidValue;
  const bool valu = gemm_mode == 1;   // 2 (split bf16) is answered by the exact float32 kernel
  if (R == 64) return valu ? launch_grad_inst<64, true>(a, ad, nwg, lds, s) : launch_grad_inst<64, false>(a, ad, nwg, lds, s);
  return valu ? launch_grad_inst<32, true>(a, ad, nwg, lds, s) : launch_grad_inst<32, false>(a, ad, nwg, lds, s);
}

template <bool VALU>
static hipError_t launch_fwd_inst(const FwdArgs& a, const ArchDims& ad, size_t lds, hipStream_t s) {
  if (const hipError_t e = allow_dynamic_lds((const void*)tower_fwd_kernel<VALU>, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((tower_fwd_kernel<VALU>), dim3((a.n + ARCH_FWD_ROWS - 1) / ARCH_FWD_ROWS, 2), dim3(TNT), lds, s, a, ad);
  return hipGetLastError();
}

// (ragged records -- a.pos_env set, rb_* the array bases -- are served: every global store of the kernel goes through rb_row)
hipError_t launch_arch_fwd(const FwdArgs& a, const ArchDims& ad, int gemm_mode, hipStream_t s) {
  if (a.nd.gauss || (a.nd.Lp != 32 && a.nd.Lp != 64) || a.n < 1) return hipErrorInvalidValue;
  if (a.pos_env && (!a.rec_mask || a.rb_T < 1)) return hipErrorInvalidValue;
  const size_t lds = arch_fwd_lds_bytes(a.nd, ad);
  if (lds > ARCH_LDS_MAX) return hipErrorInvalidValue;
  return gemm_mode == 1 ? launch_fwd_inst<true>(a, ad, lds, s) : launch_fwd_inst<false>(a, ad, lds, s);
}

// only the MFMA instantiation is built: no entry point of the grouped forward takes a gemm_mode
hipError_t launch_pool_tower(const PoolFwd& p, int K, size_t lds, hipStream_t s) {
  if (p.a.nd.gauss || (p.a.nd.Lp != 32 && p.a.nd.Lp != 64) || p.a.n < 1 || lds == 0 || lds > ARCH_LDS_MAX) return hipErrorInvalidValue;
  if (const hipError_t e = allow_dynamic_lds((const void*)pool_tower_kernel<false>, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((pool_tower_kernel<false>), dim3(pool_max_tiles(p.a.n, K), 2), dim3(TNT), lds, s, p);
  return hipGetLastError();
}

template <bool VALU>
static hipError_t launch_rollout_inst(const FwdArgs& a, const ArchDims& ad, const ScriptedSteps& sc, size_t lds, hipStream_t s) {
  if (const hipError_t e = allow_dynamic_lds((const void*)tower_rollout_kernel<VALU>, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((tower_rollout_kernel<VALU>), dim3((a.n + ARCH_FWD_ROWS - 1) / ARCH_FWD_ROWS, 2), dim3(TNT), lds, s, a, ad, sc);
  return hipGetLastError();
}

// `a`: step 0's record (rectangular, rollout-buffer row pos0 bound, no pending reward); the kernel derives the others
hipError_t launch_arch_rollout(const FwdArgs& a, const ArchDims& ad, const ScriptedSteps& sc, int gemm_mode, hipStream_t s) {
  if (a.nd.gauss || (a.nd.Lp != 32 && a.nd.Lp != 64) || a.n < 1 || a.pos_env || sc.n_steps < 1) return hipErrorInvalidValue;
  if (!a.rb_obs || !a.rb_act || !a.rb_rew || !a.rb_es || !a.rb_val || !a.rb_logp || !a.es_in || a.pending_reward) return hipErrorInvalidValue;
  if (!sc.obs_seq || !sc.rew_seq || !sc.done_seq || sc.mask_seq || a.obs != sc.obs_seq) return hipErrorInvalidValue;
  const size_t lds = arch_fwd_lds_bytes(a.nd, ad);
  if (lds > ARCH_LDS_MAX) return hipErrorInvalidValue;
  return gemm_mode == 1 ? launch_rollout_inst<true>(a, ad, sc, lds, s) : launch_rollout_inst<false>(a, ad, sc, lds, s);
}

}  // namespace ph
