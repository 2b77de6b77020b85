// C ABI of libpantheon_hip.so (see include/pantheon_hip.h for the contract and the reference call sites).
// Host side only: argument checking, workspace management, kernel launches on the context stream.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ph_launch.h"
#include "ph_block.h"
#include "ph_arch.h"
#include "ph_pool.h"
#include "ph_xplay.h"
#include "ph_record.h"
#include "ph_episode.h"
#include "ph_adap_vec.h"

namespace ph {

namespace {
// (kernel, device) pairs granted more than 64 KiB of dynamic LDS: a list that only grows at its head, under the mutex; readers walk
// it without the lock (a node's kernel and device never change, its grant only grows)
struct LdsGrant {
  const void* kernel;
  int device;
  std::atomic<size_t> bytes;
  LdsGrant* next;
};
std::atomic<LdsGrant*> lds_grants{nullptr};
std::mutex lds_grant_mutex;

LdsGrant* find_lds_grant(const void* kernel, int device) {
  for (LdsGrant* g = lds_grants.load(std::memory_order_acquire); g; g = g->next)
    if (g->kernel == kernel && g->device == device) return g;
  return nullptr;
}
}  // namespace

hipError_t allow_dynamic_lds(const void* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  int dev = 0;
  (void)hipGetDevice(&dev);
  LdsGrant* g = find_lds_grant(kernel, dev);
  if (g && g->bytes.load(std::memory_order_acquire) >= bytes) return hipSuccess;
  std::lock_guard<std::mutex> lock(lds_grant_mutex);
  if (!g && !(g = find_lds_grant(kernel, dev))) {
    g = new LdsGrant{kernel, dev, {0}, lds_grants.load(std::memory_order_relaxed)};
    lds_grants.store(g, std::memory_order_release);
  }
  if (g->bytes.load(std::memory_order_relaxed) >= bytes) return hipSuccess;   // granted by another caller meanwhile
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) g->bytes.store(bytes, std::memory_order_release);
  return e;
}

int device_cu_count() {
  static std::atomic<int> cached[64];   // per device index; 0 = not asked yet
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  const bool slot = dev >= 0 && dev < 64;
  int cu = slot ? cached[dev].load(std::memory_order_relaxed) : 0;
  if (cu > 0) return cu;
  if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) return 0;
  if (slot) cached[dev].store(cu, std::memory_order_relaxed);
  return cu;
}

}  // namespace ph

namespace {

thread_local std::string g_err;

int fail(const std::string& m) {
  g_err = m;
  return 1;
}
int fail_hip(const char* what, hipError_t e) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return 2;
}
#define PH_HIP(call)                                   \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return fail_hip(#call, _e);  \
  } while (0)

struct SpecCache {
  ph_spec spec;
  int* obs_off = nullptr;  // device prefix sums
  int* act_off = nullptr;
  int* slab_map = nullptr; // device: slab position -> parameter index for register-order gradient slabs, or null
  int* slab_map_split = nullptr;  // device: the same table for the split-bf16 gradient kernel, or null
  int* wimage_map = nullptr;      // device: parameter -> weight fragment image elements of the split kernel (ph_split.h), or null
  int split_kind = 0;             // 1 ppo_grad_split_kernel, 2 ppo_grad_split_oh_kernel, 0 neither takes the spec
  int slab_len_split = 0;         // floats per slab in that kernel's order
  int wimage_elems = 0;           // bf16 elements of its weight image
  int id = 0;                     // 1, 2, ..: position in the context's cache, never reused
};

}  // namespace

struct ph_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // workspace
  float* slabs = nullptr;
  size_t slabs_cap = 0;
  float* statpart = nullptr;
  size_t statpart_cap = 0;
  float* grad = nullptr;
  size_t grad_cap = 0;
  float* blocksq = nullptr;
  size_t blocksq_cap = 0;
  float* advstats = nullptr;
  size_t advstats_cap = 0;
  ph::AdamBias* adam_bias = nullptr;   // Adam's bias corrections of the current train() call's steps, one per minibatch (adv_finalize_kernel)
  size_t adam_bias_cap = 0;
  // ph_policy_act_host: pinned, coherent host staging the kernel accesses directly (host view, device view of the same memory)
  float* act_stage_host = nullptr;
  float* act_stage_dev = nullptr;
  size_t act_stage_cap = 0;   // floats
  // the two completion words of a one-tile ph_policy_act_host launch (coherent host memory, both views), the sequence number
  // the next launch stores, and -- while ph_policy_act_host is inside ph_policy_forward -- the words that launch should signal
  unsigned int* act_done_host = nullptr;
  unsigned int* act_done_dev = nullptr;
  unsigned int act_seq = 0;
  unsigned int* fwd_host_done = nullptr;
  int joint_reward_rule = 0;     // ph_ctx_set_joint_reward_rule: how a step's joint action enters the agents' rewards
  int wimage_zeroed_for = 0;                // spec-cache id the weight image's unbacked elements were last zeroed for (ids are never reused)
  size_t wimage_cap = 0;                    // elements allocated
  bool exclusive = false;             // ph_set_exclusive_device: nothing else runs on the device beside this context's launches
  unsigned short* wimage = nullptr;   // split gradient kernel: pre-split weight fragments of the policy being trained (ph_split.h)
  double* advpart = nullptr;     // per-segment partial sums of the advantage statistics
  size_t advpart_cap = 0;
  int* perm_idx = nullptr;   // (n_epochs, N) minibatch order of the current train() call, written by adv_stats
  size_t perm_idx_cap = 0;
  int* perm_phys = nullptr;  // the same order as physical buffer rows (t * E + e)
  size_t perm_phys_cap = 0;
  // the split gradient kernel's pack of the current train() call (ph_split.h): observation rows as bf16 planes, per-row scalars
  // of either net in minibatch order
  uint4* ximg = nullptr;     // [rows + 1][24]
  size_t ximg_cap = 0;       // in uint4
  uint4* rec_pi = nullptr;   // (n_epochs, N)
  uint4* rec_vf = nullptr;
  size_t rec_cap = 0;        // elements of each
  uint4* rowrec = nullptr;   // [rows][2] the per-row scalars packed by physical row (input of the record pass)
  size_t rowrec_cap = 0;
  // the fused reduce + clip + Adam launch of an exclusive learner (ppo_step_kernel): one stamped word per block (+ 1), the
  // launch generation, the count of sweeps that timed out
  unsigned long long* step_words = nullptr;
  size_t step_words_cap = 0;
  unsigned int* step_gen = nullptr;   // [2]: generation, sweep errors
  float* am_buf = nullptr;       // AdapPolicyMult: the dense intermediates of one net (ph_adapmult.hip), one block
  size_t am_buf_cap = 0;         // floats
  float* adap_extra = nullptr;   // [workgroups][policy-side parameters] gradient slabs of ADAP's context term
  size_t adap_extra_cap = 0;
  float* adap_loss = nullptr;    // [workgroups] partial sums of the raw term
  size_t adap_loss_cap = 0;
  float* scalars = nullptr;  // [4]
  int* stop_flag = nullptr;  // [1]
  std::vector<SpecCache> specs;
  std::vector<hipGraphExec_t> graphs;
  std::vector<int> graph_nodes;             // nodes of each captured graph (kernel, memcpy and memset nodes alike), counted at ph_graph_end
  bool capturing = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ph_p2p* p2p_dev = nullptr;      // device copy of the peer-to-peer descriptor used by the fused step launches
  ph_p2p p2p_host;                // what p2p_dev currently holds
  bool p2p_valid = false;
  void* comm = nullptr;           // ncclComm_t of the agent-per-GPU exchange (ph_comm_init), or null
  int comm_world = 1, comm_rank = 0;
  hipEvent_t ev_grad = nullptr;   // ph_ppo_train_multi: "this learner's latest gradient launch"
  int num_cu = 256;
  int exchange_blocks_per_cu = 0;           // occupancy answer for the exchange rollout kernel (0 = not asked yet)
  unsigned long long* rng_epoch = nullptr;  // caller-owned device word
  ph::RecordLog rec{};                      // ph_liar_record_attach: the move log the Liar's Dice steps fill (caller-owned arrays)
  bool recording = false;
  // partner pool (ph_pool.h): the member table the kernels read (device) with what it holds (host), the bucket pass's outputs
  ph::PoolMemberDev* pool_dev = nullptr;
  ph::PoolMemberDev pool_host[PH_MAX_POOL];
  int pool_count = 0;                       // members pool_dev holds, 0 = nothing yet
  bool pool_wide = false;                   // ... of which one is a 64-wide or a scripted member (pool_fwd16h_kernel has a tile to run)
  size_t pool_tower_lds = 0;                // ... the largest forward carve of its tower members, 0 = no tower (found at the upload)
  bool pool_adap = false;                   // ... of which one is an ADAP member (pool_adap_kernel has a tile to run)
  int* pool_order = nullptr;                // (n)
  size_t pool_order_cap = 0;
  int* pool_tiles = nullptr;                // [pool_max_tiles + 1][3]; the last record's first word is the tile count
  size_t pool_tiles_cap = 0;
  // the block worlds' grouped forward (ph_block_group_forward): a member table per seat -- [1] a constructor spec's, [0] every other
  // spec's (the planners') -- beside the Liar's Dice table above, with what each holds
  ph::PoolMemberDev* group_dev[2] = {nullptr, nullptr};
  ph::PoolMemberDev group_host[2][PH_MAX_POOL];
  int group_count[2] = {0, 0};
  bool group_scripted[2] = {false, false};  // ... of which one is scripted (launch_block_group_scripted has rows to write)
  bool group_frozen[2] = {false, false};    // ... of which one is frozen (launch_group_fwd has a tile to run)
  bool group_learner[2] = {false, false};   // ... of which one is a learner (launch_group_learn runs the tiles; the block pool only)
  long long* prof = nullptr;               // caller-owned debug stamp buffer
  double* ep_partial = nullptr;             // ph_episode_stats: [workgroups][PH_MAX_POOL][PH_EPISODE_NSTAT] partial sums of one scan
  size_t ep_partial_cap = 0;
  unsigned int* ep_ticket = nullptr;        // [1] workgroups of the scan in flight that have stored their partials (zero between launches)
  // ModularAlgorithm workspace (ph_modular_*): activations and head gradients in minibatch order, the towers' slab maps
  struct ModWs {
    float* act = nullptr;        // one allocation carved into the arrays below
    size_t act_cap = 0;
    int* maps = nullptr;         // [n_modules][n_slots][RS_NET] slab position -> parameter index, one set per trained module
    ph_spec spec;
    ph_modular mod;
    bool maps_valid = false;
    float* kl_sum = nullptr;     // [1]
    int* scratch = nullptr;      // [2 + PH_MOD_MAX] throw-away optimizer counters of ph_modular_minibatch_grad's statistics
  } mw;
};

namespace {

// Every entry point that takes a context runs with the context's device current and restores the caller's device on
// return: a process that holds models on several GPUs (or whose torch current device differs) would otherwise allocate
// workspaces and launch on whichever device happened to be current (ph_ctx_create used to leave its device selected).
struct DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(const ph_ctx* ctx) {
    if (!ctx) return;
    if (hipGetDevice(&prev) == hipSuccess && prev != ctx->device) switched = hipSetDevice(ctx->device) == hipSuccess;
  }
  ~DevGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

// grow a workspace array to n elements; never inside graph capture (the captured launches would keep the freed pointer)
template <typename T>
int ensure(const ph_ctx* ctx, T*& p, size_t& cap, size_t n) {
  if (n <= cap) return 0;
  if (ctx->capturing) return fail("workspace would grow inside graph capture: run the same call once outside capture first");
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
  if (e != hipSuccess) return fail_hip("hipMalloc(workspace)", e);
  cap = n;
  return 0;
}

int check_space(const ph_space& s, const char* name) {
  if (s.kind != PH_SPACE_BOX && s.kind != PH_SPACE_DISCRETE) return fail(std::string(name) + ": unknown space kind");
  if (s.n <= 0) return fail(std::string(name) + ": empty space");
  if (s.kind == PH_SPACE_DISCRETE) {
    if (s.n > PH_MAX_COMP) return fail(std::string(name) + ": too many components");
    for (int i = 0; i < s.n; ++i)
      if (s.nvec[i] <= 0) return fail(std::string(name) + ": nvec entries must be positive");
  }
  return 0;
}

int layout_of(const ph_spec* spec, ph_layout* o) {
  if (!spec || !o) return fail("null spec/layout");
  if (check_space(spec->obs, "observation space")) return 1;
  if (check_space(spec->act, "action space")) return 1;
  const bool gauss = spec->act.kind == PH_SPACE_BOX;   // Box actions: DiagGaussian head, A means + log_std[A] (general kernels only)
  if (gauss && spec->act.n > PH_MAX_BOX_ACT) return fail("Box action spaces: at most PH_MAX_BOX_ACT dimensions");
  o->D = spec->obs.n;
  o->F = 0;
  if (spec->obs.kind == PH_SPACE_BOX) o->F = spec->obs.n;
  else
    for (int i = 0; i < spec->obs.n; ++i) o->F += spec->obs.nvec[i];
  o->A = spec->act.n;
  o->L = 0;
  if (gauss) o->L = spec->act.n;   // the head's outputs are the A means
  else
    for (int i = 0; i < spec->act.n; ++i) o->L += spec->act.nvec[i];
  if (o->L > PH_MAX_LOGITS) return fail("too many logits (PH_MAX_LOGITS)");
  const int H = PH_HIDDEN;
  int off = 0;
  o->pi_W1 = off; off += o->F * H;
  o->pi_b1 = off; off += H;
  o->pi_W2 = off; off += H * H;
  o->pi_b2 = off; off += H;
  o->vf_W1 = off; off += o->F * H;
  o->vf_b1 = off; off += H;
  o->vf_W2 = off; off += H * H;
  o->vf_b2 = off; off += H;
  o->act_W = off; off += H * o->L;
  o->act_b = off; off += o->L;
  o->val_W = off; off += H;
  o->val_b = off; off += 1;
  if (gauss) off += o->A;   // log_std[A] (SB3 DiagGaussianDistribution.proba_distribution_net's nn.Parameter), behind val_b
  o->P = off;
  return 0;
}

// device-resident prefix sums of the nvec arrays, cached per distinct spec
// box_act_ok: the caller's kernels know the DiagGaussian head (the general forward / gradient kernels: ph_policy_forward,
// ph_ppo_minibatch_grad, ph_ppo_train); every other entry point refuses a Box action space here
int resolve(ph_ctx* ctx, const ph_spec* spec, ph::NetDims* nd, bool box_act_ok = false) {
  if (layout_of(spec, &nd->lay)) return 1;
  const bool gauss = spec->act.kind == PH_SPACE_BOX;
  if (gauss && !box_act_ok)
    return fail("Box (continuous) action spaces run on ph_policy_forward / ph_ppo_minibatch_grad / ph_ppo_train only "
                "(the DiagGaussian head lives in the general kernels)");
  SpecCache* hit = nullptr;
  for (auto& c : ctx->specs)
    if (std::memcmp(&c.spec, spec, sizeof(ph_spec)) == 0) { hit = &c; break; }
  if (!hit) {
    if (ctx->capturing) return fail("first use of a spec inside graph capture: call it once outside capture first");
    SpecCache c;
    std::memcpy(&c.spec, spec, sizeof(ph_spec));
    std::vector<int> ao(spec->act.n + 1, 0);
    for (int i = 0; i < spec->act.n; ++i) ao[i + 1] = ao[i] + (gauss ? 1 : spec->act.nvec[i]);
    PH_HIP(hipMalloc((void**)&c.act_off, ao.size() * sizeof(int)));
    PH_HIP(hipMemcpy(c.act_off, ao.data(), ao.size() * sizeof(int), hipMemcpyHostToDevice));
    if (spec->obs.kind == PH_SPACE_DISCRETE) {
      std::vector<int> oo(spec->obs.n + 1, 0);
      for (int i = 0; i < spec->obs.n; ++i) oo[i + 1] = oo[i] + spec->obs.nvec[i];
      PH_HIP(hipMalloc((void**)&c.obs_off, oo.size() * sizeof(int)));
      PH_HIP(hipMemcpy(c.obs_off, oo.data(), oo.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    {   // does this spec run on the gradient kernel with register-order slabs?  then its slab table goes to the device once
      ph::NetDims probe;
      probe.lay = nd->lay;
      probe.nchunk = (nd->lay.F + PH_HIDDEN - 1) / PH_HIDDEN;
      probe.A = nd->lay.A;
      probe.L = nd->lay.L;
      probe.F = nd->lay.F;
      probe.obs_kind = spec->obs.kind;
      probe.gauss = gauss ? 1 : 0;
      if (ph::grad_uses_reg_slabs(probe)) {
        std::vector<int> m(2 * ph::RS_NET);
        ph::grad_slab_map(nd->lay, m.data(), ph::grad_fast_fold(probe));
        PH_HIP(hipMalloc((void**)&c.slab_map, m.size() * sizeof(int)));
        PH_HIP(hipMemcpy(c.slab_map, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice));
        if (ph::grad_split_eligible(probe)) {
          ph::grad_slab_map_split(nd->lay, m.data(), ph::grad_fast_fold(probe));
          PH_HIP(hipMalloc((void**)&c.slab_map_split, m.size() * sizeof(int)));
          PH_HIP(hipMemcpy(c.slab_map_split, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice));
          std::vector<int> wm(2 * (size_t)nd->lay.P);
          ph::grad_weight_image_map(nd->lay, ph::grad_fast_fold(probe), wm.data());
          PH_HIP(hipMalloc((void**)&c.wimage_map, wm.size() * sizeof(int)));
          PH_HIP(hipMemcpy(c.wimage_map, wm.data(), wm.size() * sizeof(int), hipMemcpyHostToDevice));
          c.split_kind = 1;
          c.slab_len_split = 2 * ph::RS_NET;
          c.wimage_elems = ph::WIMG_ELEMS;
        }
      } else {
        probe.D = nd->lay.D;
        if (ph::grad_split_oh_eligible(probe)) {   // one-hot observations: the wide split kernel's tables
          std::vector<int> m((size_t)ph::grad_split_oh_slab_len(probe));
          ph::grad_slab_map_split_oh(nd->lay, probe.nchunk, m.data());
          PH_HIP(hipMalloc((void**)&c.slab_map_split, m.size() * sizeof(int)));
          PH_HIP(hipMemcpy(c.slab_map_split, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice));
          std::vector<int> wm(2 * (size_t)nd->lay.P);
          ph::grad_weight_image_map_oh(nd->lay, probe.nchunk, wm.data());
          PH_HIP(hipMalloc((void**)&c.wimage_map, wm.size() * sizeof(int)));
          PH_HIP(hipMemcpy(c.wimage_map, wm.data(), wm.size() * sizeof(int), hipMemcpyHostToDevice));
          c.split_kind = 2;
          c.slab_len_split = ph::grad_split_oh_slab_len(probe);
          c.wimage_elems = ph::grad_split_oh_wimage_elems(probe);
        }
      }
    }
    c.id = (int)ctx->specs.size() + 1;
    ctx->specs.push_back(c);
    hit = &ctx->specs.back();
  }
  nd->slab_map = hit->slab_map;
  nd->slab_map_split = hit->slab_map_split;
  nd->wimage_map = hit->wimage_map;
  nd->split = 0;
  nd->split_kind = hit->split_kind;
  nd->slab_len_split = hit->slab_len_split;
  nd->wimage_elems = hit->wimage_elems;
  nd->spec_id = hit->id;
  nd->obs_kind = spec->obs.kind;
  nd->gauss = gauss ? 1 : 0;
  nd->D = nd->lay.D;
  nd->F = nd->lay.F;
  nd->A = nd->lay.A;
  nd->L = nd->lay.L;
  nd->Lp = ((nd->L + 31) / 32) * 32;
  nd->nchunk = (nd->F + PH_HIDDEN - 1) / PH_HIDDEN;
  nd->head16 = !gauss && spec->act.n <= 4;
  for (int i = 0; i < spec->act.n && i < 4 && !gauss; ++i) nd->head16 = nd->head16 && spec->act.nvec[i] <= 16;
  nd->obs_off = hit->obs_off;
  nd->act_off = hit->act_off;
  return 0;
}

int check_rb(const ph_rollout* rb) {
  if (!rb) return fail("null rollout buffer");
  if (rb->T <= 0 || rb->E <= 0) return fail("rollout buffer: T and E must be positive");
  if (!rb->observations || !rb->actions || !rb->rewards || !rb->episode_starts || !rb->values || !rb->log_probs ||
      !rb->advantages || !rb->returns)
    return fail("rollout buffer: null array");
  if ((long long)rb->T * rb->E >= (1ll << 31)) return fail("rollout buffer: T*E must fit in int32");
  return 0;
}

int fail_who(const char* who, const char* what) { return fail(std::string(who) + what); }
// what the 16-byte accesses of a Liar's Dice table's state need, in the words of every entry point that takes one
const char* const LIAR_ALIGN16 = ": hands/history must be 16-byte aligned";

int arch_resolve(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, ph::NetDims* nd, ph::ArchDims* ad);   // with the towers, below
int arch_host_dims(const ph_spec* spec, const ph_arch* arch, ph::NetDims* nd, ph::ArchDims* ad);
int arch_lds_refusal(const ph::NetDims& nd, const ph::ArchDims& ad);

// a zeroed forward record with the spec resolved and the fields every forward entry point sets: for the 64-wide kernels (null
// arch), or for the towers of `arch`, whose dimensions go to `ad` (arch_resolve: no Box actions, the LDS refusal, lay.P the arch's)
int fwd_args(ph::FwdArgs& a, ph_ctx* ctx, const ph_spec* spec, bool box_act_ok, const float* params, const float* obs, int n,
             unsigned long long seed, unsigned long long counter, int* act_i32, float* values, float* logp,
             const ph_arch* arch = nullptr, ph::ArchDims* ad = nullptr) {
  std::memset(&a, 0, sizeof(a));
  if (arch ? arch_resolve(ctx, spec, arch, &a.nd, ad) : resolve(ctx, spec, &a.nd, box_act_ok)) return 1;
  a.params = params;
  a.obs = obs;
  a.n = n;
  a.seed = seed;
  a.counter = counter;
  a.epoch = ctx->rng_epoch;
  a.act_i32 = act_i32;
  a.values = values;
  a.logp = logp;
  return 0;
}

// the fused RolloutBuffer.add of a forward record: row `pos` of `rb` (none when rb is null), and pending_reward added to the
// previous row's rewards (Agent.update folded into the next step's launch); messages name the entry point `who`
int fwd_bind_row(const char* who, ph::FwdArgs& a, const ph_rollout* rb, int pos, const float* episode_start_in,
                 const float* pending_reward) {
  if (!rb) return pending_reward ? fail_who(who, ": pending_reward needs the fused rollout-buffer write") : 0;
  if (check_rb(rb)) return 1;
  if (a.n != rb->E) return fail_who(who, ": fused add needs n == rollout E");
  if (pos < 0 || pos >= rb->T) return fail_who(who, ": pos out of range (buffer full?)");
  if (!episode_start_in) return fail_who(who, ": fused add needs episode_start_in");
  const size_t row = (size_t)pos * rb->E;
  a.rb_obs = rb->observations + row * a.nd.D;
  a.rb_act = rb->actions + row * a.nd.A;
  a.rb_rew = rb->rewards + row;
  a.rb_es = rb->episode_starts + row;
  a.rb_val = rb->values + row;
  a.rb_logp = rb->log_probs + row;
  a.es_in = episode_start_in;
  if (pending_reward) {
    if (pos < 1) return fail_who(who, ": pending_reward needs pos >= 1");
    a.prev_rew = rb->rewards + (row - rb->E);
    a.pending_reward = pending_reward;
  }
  return 0;
}
// its ragged sibling: the array bases of a checked `rb`, the kernel selecting each env's row -- with pos_env the row pos_env[e] where
// rec_mask[e] (ragged forwards), without it a row the kernel walks itself (one-launch rollouts)
void fwd_bind_bases(ph::FwdArgs& a, const ph_rollout* rb, const float* es_in, const int* pos_env, const unsigned char* rec_mask) {
  a.rb_obs = rb->observations;
  a.rb_act = rb->actions;
  a.rb_rew = rb->rewards;
  a.rb_es = rb->episode_starts;
  a.rb_val = rb->values;
  a.rb_logp = rb->log_probs;
  a.es_in = es_in;
  if (!pos_env) return;
  a.pos_env = pos_env;
  a.rec_mask = rec_mask;
  a.rb_T = rb->T;
}

// what an evaluating forward takes and returns besides the sampled step
void fwd_eval_fields(ph::FwdArgs& a, const unsigned char* mask, const float* uniforms, const float* given_actions, int deterministic,
                     float* act_f32, float* entropy, float* logits) {
  a.mask = mask;
  a.uniforms = uniforms;
  a.given_actions = given_actions;
  a.deterministic = deterministic;
  a.act_f32 = act_f32;
  a.entropy = entropy;
  a.logits = logits;
}

// The three forward entry points, each written once: on the 64-wide kernels (null arch) or on the towers of `arch`.  Messages name
// the entry point `who`.
int forward_run(const char* who, ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params, const float* obs, int n,
                const unsigned char* action_mask, const float* uniforms, const float* given_actions, unsigned long long seed,
                unsigned long long counter, int deterministic, int* actions_i32, float* actions_f32, float* values, float* log_probs,
                float* entropy, float* logits, const ph_rollout* rb, int pos, const float* episode_start_in,
                const float* pending_reward, int gemm_mode) {
  if (!ctx) return fail("null ctx");
  if (!params || !obs) return fail_who(who, ": null params/obs");
  if ((uintptr_t)params % 16 != 0) return fail_who(who, ": params must be 16-byte aligned");
  if (n <= 0) return fail_who(who, ": n must be positive");
  ph::FwdArgs a;
  ph::ArchDims ad;
  // Box actions: the 64-wide forward knows the DiagGaussian head; a tower refuses them whatever is said here
  if (fwd_args(a, ctx, spec, true, params, obs, n, seed, counter, actions_i32, values, log_probs, arch, &ad)) return 1;
  if (a.nd.gauss && action_mask) return fail_who(who, ": action masks belong to the categorical heads");
  fwd_eval_fields(a, action_mask, uniforms, given_actions, deterministic, actions_f32, entropy, logits);
  a.prof = ctx->prof;
  if (fwd_bind_row(who, a, rb, pos, episode_start_in, pending_reward)) return 1;
  if (arch) {
    PH_HIP(ph::launch_arch_fwd(a, ad, gemm_mode, ctx->stream));
    return 0;
  }
  a.host_done = ctx->fwd_host_done;   // ph_policy_act_host's arrival words: the 64-wide forward only
  a.host_seq = ctx->act_seq;
  PH_HIP(ph::launch_policy_fwd(a, gemm_mode, ctx->stream));
  return 0;
}

int forward_ragged_run(const char* who, ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params, const float* obs,
                       const unsigned char* action_mask, unsigned long long seed, unsigned long long counter, int deterministic,
                       int* actions_i32, float* values, float* log_probs, const ph_rollout* rb, const int* pos_env,
                       const unsigned char* record_mask, const float* episode_start_in, int gemm_mode) {
  if (!ctx) return fail("null ctx");
  if (!params || !obs || !pos_env || !record_mask || !episode_start_in) return fail_who(who, ": null argument");
  if ((uintptr_t)params % 16 != 0) return fail_who(who, ": params must be 16-byte aligned");
  if (check_rb(rb)) return 1;
  ph::FwdArgs a;
  ph::ArchDims ad;
  if (fwd_args(a, ctx, spec, false, params, obs, rb->E, seed, counter, actions_i32, values, log_probs, arch, &ad)) return 1;
  a.mask = action_mask;
  a.prof = ctx->prof;
  a.deterministic = deterministic;
  fwd_bind_bases(a, rb, episode_start_in, pos_env, record_mask);
  PH_HIP(arch ? ph::launch_arch_fwd(a, ad, gemm_mode, ctx->stream) : ph::launch_policy_fwd(a, gemm_mode, ctx->stream));
  return 0;
}

int scripted_rollout_run(const char* who, ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params,
                         const float* obs_seq, const float* rew_seq, const float* done_seq, int n, int n_steps,
                         const float* episode_start0, unsigned long long seed, unsigned long long counter0, int* actions_i32,
                         float* values, float* log_probs, const ph_rollout* rb, int pos0, int gemm_mode) {
  if (!ctx) return fail("null ctx");
  if (!params || !obs_seq || !rew_seq || !done_seq || !episode_start0) return fail_who(who, ": null argument");
  if ((uintptr_t)params % 16 != 0) return fail_who(who, ": params must be 16-byte aligned");
  if (n <= 0 || n_steps <= 0) return fail_who(who, ": n and n_steps must be positive");
  if (check_rb(rb)) return 1;
  if (n != rb->E) return fail_who(who, ": n must equal the rollout buffer's E");
  if (pos0 < 0 || pos0 > rb->T - n_steps) return fail_who(who, ": rows pos0 .. pos0 + n_steps - 1 must lie in the buffer");
  ph::FwdArgs a;
  ph::ArchDims ad;
  if (fwd_args(a, ctx, spec, false, params, obs_seq, n, seed, counter0, actions_i32, values, log_probs, arch, &ad)) return 1;
  if (!arch && !ph::fwd16_eligible(a.nd, n))
    return fail_who(who, ": needs the 16-row forward's shape class (one feature chunk, one Discrete head of <= 8 logits, "
                         "n < 16384); use ph_policy_forward per step");
  a.prof = ctx->prof;
  if (fwd_bind_row(who, a, rb, pos0, episode_start0, nullptr)) return 1;   // step 0's row
  ph::ScriptedSteps sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.n_steps = n_steps;
  sc.obs_seq = obs_seq;
  sc.rew_seq = rew_seq;
  sc.done_seq = done_seq;
  PH_HIP(arch ? ph::launch_arch_rollout(a, ad, sc, gemm_mode, ctx->stream)
              : ph::launch_policy_fwd16_rollout(a, sc, gemm_mode, ctx->stream));
  return 0;
}

// The advantage-statistics record of n_mb minibatches per epoch walking a permutation of the buffer's N rows: `perms`, or the
// keyed Feistel order of perm_seed materialised into perm_idx; the order once more as physical rows into perm_phys (the tile
// walk then has no index arithmetic).  No row records and no stop-flag reset: callers add what their launches read.
ph::AdvStatArgs adv_args_epochs(const ph_ctx* ctx, const ph_rollout* rb, const int* perms, unsigned long long perm_seed, int batch,
                                int n_mb) {
  const int N = rb->T * rb->E;
  ph::AdvStatArgs aa{};
  aa.rb_adv = rb->advantages;
  aa.T = rb->T;
  aa.E = rb->E;
  aa.perms = perms;
  aa.perm_n = (uint32_t)N;
  aa.perm_hb = ph::feistel_half_bits((uint32_t)N);
  aa.perm_seed = perm_seed;
  aa.epoch = ctx->rng_epoch;
  aa.N = N;
  aa.batch = batch;
  aa.n_mb = n_mb;
  aa.out = ctx->advstats;
  aa.partial = ctx->advpart;
  aa.idx_out = perms ? nullptr : ctx->perm_idx;
  aa.phys_out = ctx->perm_phys;
  return aa;
}
// the same for one minibatch given as indices[0..nb): one "epoch" whose first nb entries are the minibatch
ph::AdvStatArgs adv_args_minibatch(const ph_ctx* ctx, const ph_rollout* rb, const int* indices, int nb) {
  ph::AdvStatArgs aa{};
  aa.rb_adv = rb->advantages;
  aa.T = rb->T;
  aa.E = rb->E;
  aa.perms = indices;
  aa.perm_hb = 1;
  aa.N = nb;
  aa.batch = nb;
  aa.n_mb = 1;
  aa.out = ctx->advstats;
  aa.partial = ctx->advpart;
  aa.phys_out = ctx->perm_phys;
  return aa;
}

// minibatch mbi = ep * n_mb + k of n_mb minibatches per epoch over N rows: positions [start, start + nb) of epoch ep's order,
// whose indices begin at idx (`perms`, or the order the advantage-statistics launch materialised into perm_idx)
struct MbWalk {
  int ep, start, nb;
  const int* idx;
};
MbWalk minibatch_walk(const ph_ctx* ctx, const int* perms, int N, int n_mb, int batch_size, int mbi) {
  MbWalk w;
  w.ep = mbi / n_mb;
  w.start = (mbi - w.ep * n_mb) * batch_size;
  w.nb = N - w.start < batch_size ? N - w.start : batch_size;
  w.idx = (perms ? perms : ctx->perm_idx) + (size_t)w.ep * N + w.start;
  return w;
}

// The reduce record of one minibatch: nslab gradient slabs of slab_len floats (`map`: slab position -> parameter index, null =
// canonical order) and 2 * nslab statistics partials -> grad[P] and stats_out.  With `opt` a train() call's KL decision and step
// counter; without it a plain gradient (no KL stop, no step).
ph::ReduceArgs reduce_args(const ph_ctx* ctx, const ph_ppo_hyper* hp, const ph_opt_state* opt, int P, int slab_len, const int* map,
                           int nslab, int nb, float* grad, float* stats_out) {
  ph::ReduceArgs r;
  r.slabs = ctx->slabs;
  r.nslab = nslab;
  r.nstatpart = 2 * nslab;
  r.P = P;
  r.slab_len = slab_len;
  r.map = map;
  r.grad = grad;
  r.blocksq = ctx->blocksq;
  r.statpart = ctx->statpart;
  r.stats_out = stats_out;
  r.nb = nb;
  r.ent_coef = hp->ent_coef;
  r.vf_coef = hp->vf_coef;
  r.target_kl = opt ? hp->target_kl : -1.f;
  r.stop_flag = ctx->stop_flag;
  r.step = opt ? opt->step : nullptr;
  r.scalars = ctx->scalars;
  return r;
}
// the clip + Adam record of a train() call's minibatch, on the gradient the reduction of slab_len-float slabs left in ctx->grad;
// `wimage`: the split kernel's weight image kept in step with the parameters, or null
ph::AdamArgs adam_args(const ph_ctx* ctx, const ph_ppo_hyper* hp, const ph_opt_state* opt, int P, int slab_len, float* stats_out,
                       unsigned short* wimage, const int* wimage_map) {
  ph::AdamArgs ad;
  ad.params = opt->params;
  ad.m = opt->adam_m;
  ad.v = opt->adam_v;
  ad.grad = ctx->grad;
  ad.blocksq = ctx->blocksq;
  ad.nblk = ph::reduce_blocks(slab_len);
  ad.P = P;
  ad.step = opt->step;
  ad.scalars = ctx->scalars;
  ad.stop_flag = ctx->stop_flag;
  ad.lr = hp->learning_rate;
  ad.beta1 = hp->adam_beta1;
  ad.beta2 = hp->adam_beta2;
  ad.eps = hp->adam_eps;
  ad.max_norm = hp->max_grad_norm;
  ad.stats_out = stats_out;
  ad.wimage = wimage;
  ad.wimage_map = wimage_map;
  return ad;
}

// the checks of a train() entry point's optimizer state, hyper-parameters and sizes; messages name the entry point `who`.
// `aligned`: the caller's kernels need 16-byte aligned parameters.
int check_train_call(const char* who, const ph_ctx* ctx, const ph_opt_state* opt, const ph_ppo_hyper* hp, int n_epochs,
                     int batch_size, bool aligned = true) {
  const std::string w(who);
  if (!ctx) return fail("null ctx");
  if (!opt || !opt->params || !opt->adam_m || !opt->adam_v || !opt->step) return fail(w + ": null optimizer state");
  if (aligned && (uintptr_t)opt->params % 16 != 0) return fail(w + ": params must be 16-byte aligned");
  if (!hp) return fail(w + ": null hyper-parameters");
  if (n_epochs <= 0 || batch_size <= 0) return fail(w + ": n_epochs and batch_size must be positive");
  return 0;
}
// the same for a one-minibatch gradient entry point
int check_minibatch_call(const char* who, const ph_ctx* ctx, const float* params, const ph_rollout* rb, const ph_ppo_hyper* hp,
                         const int* indices, int nb, const float* grad_out, bool aligned = true) {
  const std::string w(who);
  if (!ctx) return fail("null ctx");
  if (!params || !hp || !indices || !grad_out) return fail(w + ": null argument");
  if (aligned && (uintptr_t)params % 16 != 0) return fail(w + ": params must be 16-byte aligned");
  if (check_rb(rb)) return 1;
  if (nb <= 0) return fail(w + ": nb must be positive");
  return 0;
}

// average milliseconds of one fn(i) (0 = success) over reps calls i = 0 .. reps-1, timed by the context's events on its stream
// after `warm` untimed calls fn(0 .. warm-1)
template <typename F>
int time_reps(ph_ctx* ctx, int warm, int reps, F&& fn, float* avg_ms) {
  for (int i = 0; i < warm; ++i)
    if (fn(i)) return 1;
  PH_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  for (int i = 0; i < reps; ++i)
    if (fn(i)) return 1;
  PH_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  PH_HIP(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  PH_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *avg_ms = ms / (float)reps;
  return 0;
}
int hip_rc(hipError_t e, const char* what) { return e == hipSuccess ? 0 : fail_hip(what, e); }

}  // namespace

extern "C" {

int ph_abi_version(void) { return PH_ABI_VERSION; }
const char* ph_last_error(void) { return g_err.c_str(); }

int ph_device_count(int* n_out) {
  if (!n_out) return fail("null n_out");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *n_out = 0;
    return fail_hip("hipGetDeviceCount", e);
  }
  *n_out = n;
  return 0;
}

int ph_ctx_create(int device, ph_ctx** out) {
  if (!out) return fail("null out");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail("no HIP device visible: the PantheonRL MI355X engine has no CPU fallback");
  if (device < 0 || device >= n) return fail("device index out of range");
  ph_ctx probe;                    // the caller's current device is restored on every return path
  probe.device = device;
  DevGuard dev_guard(&probe);
  hipDeviceProp_t prop;
  PH_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 (MI355X) only");
  ph_ctx* c = new ph_ctx();
  c->device = device;
  c->num_cu = prop.multiProcessorCount;
  if (hipMalloc((void**)&c->scalars, 4 * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&c->stop_flag, sizeof(int)) != hipSuccess) {
    delete c;
    return fail("hipMalloc(ctx scalars) failed");
  }
  (void)hipMemset(c->scalars, 0, 4 * sizeof(float));
  (void)hipMemset(c->stop_flag, 0, sizeof(int));
  (void)hipEventCreate(&c->ev0);
  (void)hipEventCreate(&c->ev1);
  *out = c;
  return 0;
}

int ph_ctx_destroy(ph_ctx* ctx) {
  DevGuard dev_guard(ctx);
  if (!ctx) return 0;
  (void)hipStreamSynchronize(ctx->stream);
  for (auto g : ctx->graphs)
    if (g) (void)hipGraphExecDestroy(g);
  for (auto& s : ctx->specs) {
    if (s.obs_off) (void)hipFree(s.obs_off);
    if (s.slab_map) (void)hipFree(s.slab_map);
    if (s.slab_map_split) (void)hipFree(s.slab_map_split);
    if (s.wimage_map) (void)hipFree(s.wimage_map);
    if (s.act_off) (void)hipFree(s.act_off);
  }
  void* ptrs[] = {ctx->wimage, ctx->mw.act, ctx->mw.maps, ctx->mw.kl_sum, ctx->mw.scratch, ctx->advpart, ctx->p2p_dev, ctx->slabs, ctx->statpart, ctx->grad, ctx->blocksq, ctx->advstats, ctx->adam_bias, ctx->perm_idx, ctx->perm_phys, ctx->ximg, ctx->rec_pi, ctx->rec_vf, ctx->rowrec, ctx->step_words, ctx->step_gen, ctx->scalars, ctx->stop_flag,
                  ctx->adap_extra, ctx->adap_loss, ctx->am_buf, ctx->pool_dev, ctx->pool_order, ctx->pool_tiles, ctx->ep_partial, ctx->ep_ticket,
                  ctx->group_dev[0], ctx->group_dev[1]};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (ctx->act_stage_host) (void)hipHostFree(ctx->act_stage_host);
  if (ctx->act_done_host) (void)hipHostFree(ctx->act_done_host);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->ev_grad) (void)hipEventDestroy(ctx->ev_grad);
  (void)ph_comm_destroy(ctx);
  delete ctx;
  return 0;
}

int ph_ctx_set_joint_reward_rule(ph_ctx* ctx, int rule) {
  if (!ctx) return fail("null ctx");
  if (rule != PH_JOINT_MATCH_BONUS && rule != PH_JOINT_RPS) return fail("ph_ctx_set_joint_reward_rule: unknown rule");
  ctx->joint_reward_rule = rule;
  return 0;
}

int ph_ctx_set_stream(ph_ctx* ctx, void* hip_stream) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  ctx->stream = (hipStream_t)hip_stream;
  return 0;
}

int ph_ctx_sync(ph_ctx* ctx) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int ph_graph_begin(ph_ctx* ctx) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (ctx->capturing) return fail("already capturing");
  if (ctx->stream == nullptr) return fail("graph capture needs a non-default stream (ph_ctx_set_stream)");
  PH_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
  ctx->capturing = true;
  return 0;
}

int ph_graph_end(ph_ctx* ctx, int* graph_id_out) {
  DevGuard dev_guard(ctx);
  if (!ctx || !graph_id_out) return fail("null ctx/graph_id_out");
  if (!ctx->capturing) return fail("not capturing");
  ctx->capturing = false;
  hipGraph_t g = nullptr;
  PH_HIP(hipStreamEndCapture(ctx->stream, &g));
  hipGraphExec_t ge = nullptr;
  size_t nodes = 0;
  (void)hipGraphGetNodes(g, nullptr, &nodes);
  hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return fail_hip("hipGraphInstantiate", e);
  ctx->graphs.push_back(ge);
  ctx->graph_nodes.push_back((int)nodes);
  *graph_id_out = (int)ctx->graphs.size() - 1;
  return 0;
}

int ph_graph_nodes(ph_ctx* ctx, int graph_id, int* nodes_out) {
  if (!ctx || !nodes_out) return fail("null ctx/nodes_out");
  if (graph_id < 0 || graph_id >= (int)ctx->graph_nodes.size()) return fail("bad graph id");
  *nodes_out = ctx->graph_nodes[graph_id];
  return 0;
}

int ph_graph_launch(ph_ctx* ctx, int graph_id) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (graph_id < 0 || graph_id >= (int)ctx->graphs.size()) return fail("bad graph id");
  PH_HIP(hipGraphLaunch(ctx->graphs[graph_id], ctx->stream));
  return 0;
}

int ph_ctx_set_rng_epoch(ph_ctx* ctx, unsigned long long* epoch_dev) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  ctx->rng_epoch = epoch_dev;
  return 0;
}
int ph_rng_epoch_advance(ph_ctx* ctx) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!ctx->rng_epoch) return fail("ph_rng_epoch_advance: no epoch word attached");
  PH_HIP(ph::launch_epoch_advance(ctx->rng_epoch, ctx->stream));
  return 0;
}

int ph_debug_set_profile_buffer(ph_ctx* ctx, long long* stamps_dev) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  ctx->prof = stamps_dev;
  return 0;
}

int ph_debug_weight_image_mismatches(ph_ctx* ctx, const ph_spec* spec, const float* params, int* mismatches_host) {
  DevGuard dev_guard(ctx);
  if (!ctx || !params || !mismatches_host) return fail("ph_debug_weight_image_mismatches: null argument");
  ph::NetDims nd;
  if (resolve(ctx, spec, &nd)) return 1;
  *mismatches_host = -1;                       // -1: this context holds no image (the split kernel never ran for it)
  if (!ctx->wimage || !nd.wimage_map) return 0;
  int* d = nullptr;
  PH_HIP(hipMalloc((void**)&d, sizeof(int)));
  PH_HIP(hipMemsetAsync(d, 0, sizeof(int), ctx->stream));
  PH_HIP(ph::launch_weight_image_check(params, ctx->wimage, nd.wimage_map, nd.lay.P, d, ctx->stream));
  PH_HIP(hipMemcpyAsync(mismatches_host, d, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  (void)hipFree(d);
  return 0;
}

int ph_set_exclusive_device(ph_ctx* ctx, int exclusive) {
  if (!ctx) return fail("null ctx");
  ctx->exclusive = exclusive != 0;
  return 0;
}

int ph_ctx_step_errors(ph_ctx* ctx, unsigned int* count_out) {
  DevGuard dev_guard(ctx);
  if (!ctx || !count_out) return fail("ph_ctx_step_errors: null argument");
  *count_out = 0u;
  if (!ctx->step_gen) return 0;   // the fused step never ran on this context
  PH_HIP(hipMemcpyAsync(count_out, ctx->step_gen + 1, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
  PH_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int ph_timer_start(ph_ctx* ctx) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  PH_HIP(hipEventRecord(ctx->ev0, ctx->stream));
  return 0;
}
int ph_timer_stop(ph_ctx* ctx, float* ms_out) {
  DevGuard dev_guard(ctx);
  if (!ctx || !ms_out) return fail("null ctx/ms_out");
  PH_HIP(hipEventRecord(ctx->ev1, ctx->stream));
  PH_HIP(hipEventSynchronize(ctx->ev1));
  PH_HIP(hipEventElapsedTime(ms_out, ctx->ev0, ctx->ev1));
  return 0;
}

int ph_layout_of(const ph_spec* spec, ph_layout* out) { return layout_of(spec, out); }

// Host-only: the two tables that tie ppo_grad_split_kernel's register and fragment orders to parameter indices, for inspection
// (tests/test_host_logic.py checks them against the layout without a GPU).  Returns 0 and *eligible = 0 for specs the kernel
// does not take (the tables are then untouched).
int ph_debug_split_tables(const ph_spec* spec, int* slab_map /* 2 * 8960 */, int* image_map /* 2 * P */, int* eligible) {
  if (!spec || !slab_map || !image_map || !eligible) return fail("ph_debug_split_tables: null argument");
  ph_layout lay;
  if (layout_of(spec, &lay)) return 1;
  ph::NetDims probe;
  std::memset(&probe, 0, sizeof(probe));
  probe.lay = lay;
  probe.nchunk = (lay.F + PH_HIDDEN - 1) / PH_HIDDEN;
  probe.A = lay.A;
  probe.L = lay.L;
  probe.F = lay.F;
  probe.obs_kind = spec->obs.kind;
  *eligible = ph::grad_split_eligible(probe) ? 1 : 0;
  if (!*eligible) return 0;
  ph::grad_slab_map_split(lay, slab_map, ph::grad_fast_fold(probe));
  ph::grad_weight_image_map(lay, ph::grad_fast_fold(probe), image_map);
  return 0;
}

// The same for ppo_grad_split_oh_kernel (one-hot observations): *slab_len_out = floats per slab (both nets), *image_elems_out = bf16
// elements of its weight image; slab_map needs *slab_len_out ints (call once with slab_map = image_map = null to learn the sizes).
int ph_debug_split_oh_tables(const ph_spec* spec, int* slab_map, int* image_map /* 2 * P */, int* slab_len_out, int* image_elems_out,
                             int* eligible) {
  if (!spec || !slab_len_out || !image_elems_out || !eligible) return fail("ph_debug_split_oh_tables: null argument");
  ph_layout lay;
  if (layout_of(spec, &lay)) return 1;
  ph::NetDims probe;
  std::memset(&probe, 0, sizeof(probe));
  probe.lay = lay;
  probe.nchunk = (lay.F + PH_HIDDEN - 1) / PH_HIDDEN;
  probe.A = lay.A;
  probe.L = lay.L;
  probe.F = lay.F;
  probe.D = lay.D;
  probe.obs_kind = spec->obs.kind;
  *eligible = ph::grad_split_oh_eligible(probe) ? 1 : 0;
  if (!*eligible) return 0;
  *slab_len_out = ph::grad_split_oh_slab_len(probe);
  *image_elems_out = ph::grad_split_oh_wimage_elems(probe);
  if (slab_map) ph::grad_slab_map_split_oh(lay, probe.nchunk, slab_map);
  if (image_map) ph::grad_weight_image_map_oh(lay, probe.nchunk, image_map);
  return 0;
}

// ---- K1 ----
int ph_buffer_add(ph_ctx* ctx, const ph_spec* spec, const ph_rollout* rb, int pos, const float* obs,
                  const float* actions, const float* episode_start, const float* values, const float* log_probs) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  ph_layout lay;
  if (layout_of(spec, &lay) || check_rb(rb)) return 1;
  if (pos < 0 || pos >= rb->T) return fail("ph_buffer_add: pos out of range (buffer full?)");
  if (!obs || !actions || !episode_start || !values || !log_probs) return fail("ph_buffer_add: null input");
  const size_t E = rb->E, row = (size_t)pos * E;
  PH_HIP(ph::launch_buffer_add(rb->observations + row * lay.D, rb->actions + row * lay.A, rb->rewards + row,
                               rb->episode_starts + row, rb->values + row, rb->log_probs + row, obs, actions,
                               episode_start, values, log_probs, rb->E, lay.D, lay.A, ctx->stream));
  return 0;
}

int ph_buffer_compact_columns(ph_ctx* ctx, const ph_spec* spec, const ph_rollout* src, const ph_rollout* dst,
                              const int* cols, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  ph_layout lay;
  if (layout_of(spec, &lay) || check_rb(src) || check_rb(dst)) return 1;
  if (!cols || n <= 0 || n > src->E) return fail("ph_buffer_compact_columns: bad column list");
  if (dst->T != src->T || dst->E != n) return fail("ph_buffer_compact_columns: destination must be (T, n)");
  PH_HIP(ph::launch_buffer_compact(*src, *dst, cols, n, lay.D, lay.A, ctx->stream));
  return 0;
}

int ph_buffer_add_reward(ph_ctx* ctx, const ph_rollout* rb, int pos, const float* reward,
                         const unsigned char* env_mask) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (check_rb(rb)) return 1;
  if (pos < 0 || pos >= rb->T) return fail("ph_buffer_add_reward: pos out of range");
  if (!reward) return fail("ph_buffer_add_reward: null reward");
  PH_HIP(ph::launch_reward_add(rb->rewards + (size_t)pos * rb->E, reward, env_mask, rb->E, ctx->stream));
  return 0;
}

int ph_buffer_add_reward_const(ph_ctx* ctx, const ph_rollout* rb, int pos, float reward) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (check_rb(rb)) return 1;
  if (pos < 0 || pos >= rb->T) return fail("ph_buffer_add_reward_const: pos out of range");
  PH_HIP(ph::launch_reward_add_const(rb->rewards + (size_t)pos * rb->E, reward, rb->E, ctx->stream));
  return 0;
}

int ph_buffer_add_reward_joint(ph_ctx* ctx, const ph_rollout* rb, int pos, const float* base_reward,
                               const int* joint_actions, int n_seats, int seat, const int* partner_seat, float bonus) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (check_rb(rb)) return 1;
  if (pos < 0 || pos >= rb->T) return fail("ph_buffer_add_reward_joint: pos out of range");
  if (!base_reward || !joint_actions || !partner_seat) return fail("ph_buffer_add_reward_joint: null argument");
  if (n_seats <= 0 || seat < 0 || seat >= n_seats) return fail("ph_buffer_add_reward_joint: bad seat");
  PH_HIP(ph::launch_reward_add_joint(rb->rewards + (size_t)pos * rb->E, base_reward, joint_actions, rb->E, n_seats, seat,
                                     partner_seat, bonus, ctx->joint_reward_rule, ctx->stream));
  return 0;
}

int ph_roundrobin_env_step(ph_ctx* ctx, const int* joint_actions, int* partnerid, const float* base_reward, const float* done,
                           float* reward_out, int* alt_action_out, float* next_block, int block_ld, int n_partners,
                           float bonus, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!joint_actions || !partnerid || !base_reward || !done || !reward_out)
    return fail("ph_roundrobin_env_step: null argument");
  if (n <= 0 || n_partners <= 0) return fail("ph_roundrobin_env_step: bad sizes");
  if (next_block && block_ld < 3) return fail("ph_roundrobin_env_step: routing block rows need >= 3 header columns");
  PH_HIP(ph::launch_roundrobin_env_step(joint_actions, partnerid, base_reward, done, reward_out, alt_action_out, next_block,
                                        block_ld, n_partners, bonus, n, ctx->stream));
  return 0;
}

// ---- engine-side round-robin layout (config 4) -------------------------------------------------------------------------------
namespace {
constexpr size_t RR_STAMP_BYTES = 64 * sizeof(unsigned long long);
size_t rr_slot_bytes(int n_partners, int n, int block_ld) {
  const size_t blk = (size_t)n * (block_ld + 1) * sizeof(float), act = (size_t)(n_partners + 1) * n * sizeof(int);
  return ((blk > act ? blk : act) + 255) / 256 * 256;
}
int check_rr_link(const ph_rr_link* l) {
  if (!l) return fail("null ph_rr_link");
  if (l->n_partners < 1 || l->n_partners + 1 > PH_MAX_RANKS) return fail("ph_rr_link: n_partners out of range");
  if (l->rank < 0 || l->rank > l->n_partners || l->n <= 0 || l->block_ld <= 3) return fail("ph_rr_link: bad rank / n / block_ld");
  if (!l->error) return fail("ph_rr_link: error word required");
  for (int r = 0; r <= l->n_partners; ++r)
    if (!l->area[r]) return fail("ph_rr_link: unmapped peer area");
  return 0;
}
unsigned long long* rr_stamps(const ph_rr_link* l, int rank) { return (unsigned long long*)l->area[rank]; }
// rank 0's arrival counters of the block send live behind its stamp words (words 32 .. 63 of the stamp area)
unsigned int* rr_arrive(const ph_rr_link* l) { return (unsigned int*)((unsigned long long*)l->area[0] + 32); }
char* rr_slot(const ph_rr_link* l, int rank, int parity) {
  return (char*)l->area[rank] + RR_STAMP_BYTES + (size_t)parity * rr_slot_bytes(l->n_partners, l->n, l->block_ld);
}
}  // namespace

int ph_rr_area_bytes(int n_partners, int n, int block_ld, size_t* bytes_out) {
  if (!bytes_out || n_partners < 1 || n <= 0 || block_ld <= 3) return fail("ph_rr_area_bytes: bad argument");
  *bytes_out = RR_STAMP_BYTES + 2 * rr_slot_bytes(n_partners, n, block_ld);
  return 0;
}

int ph_roundrobin_ego_iteration(ph_ctx* ctx, const ph_rr_link* link, const ph_rr_ego* ego, int T, unsigned long long iteration) {
  DevGuard dev_guard(ctx);
  if (!ctx || !ego || T <= 0) return fail("ph_roundrobin_ego_iteration: bad argument");
  if (check_rr_link(link)) return 1;
  if (link->rank != 0) return fail("ph_roundrobin_ego_iteration: the ego lives on rank 0");
  if (!ego->params || !ego->obs_seq || !ego->base_reward_seq || !ego->done_seq || !ego->blocks || !ego->partnerid ||
      !ego->rewards || !ego->episode_start0 || !ego->rb)
    return fail("ph_roundrobin_ego_iteration: null argument");
  if (check_rb(ego->rb)) return 1;
  if (ego->rb->E != link->n || ego->rb->T < T) return fail("ph_roundrobin_ego_iteration: rollout buffer shape");
  ph::NetDims nd;
  if (resolve(ctx, ego->spec, &nd)) return 1;
  const int n = link->n, K = link->n_partners, ld = link->block_ld;
  for (int t = 0; t < T; ++t) {
    const unsigned long long want = iteration * (unsigned long long)T + (unsigned long long)t + 1ull;
    int* slot = (int*)rr_slot(link, 0, t & 1);   // (1 + K, n): row 0 = the ego's actions of this step
    // the routing block leaves first: the partners work on step t while the ego's own forward runs
    ph::RRSend sd;
    std::memset(&sd, 0, sizeof(sd));
    sd.src = ego->blocks + (size_t)t * n * ld;
    sd.n = n;
    sd.block_ld = ld;
    for (int k = 0; k < K; ++k) {
      sd.dst[k] = (float*)rr_slot(link, 1 + k, t & 1);
      sd.stamp[k] = rr_stamps(link, 1 + k);
    }
    sd.arrive = rr_arrive(link);
    sd.want = want;
    PH_HIP(ph::launch_rr_send_block(sd, K, ctx->stream));
    if (ph_policy_forward(ctx, ego->spec, ego->params, ego->obs_seq + (size_t)t * n * nd.D, n, nullptr, nullptr, nullptr, ego->seed,
                          ego->counter0 + (unsigned long long)t, 0, slot, nullptr, ego->values, ego->log_probs, nullptr, nullptr,
                          ego->rb, t, t == 0 ? ego->episode_start0 : ego->done_seq + (size_t)(t - 1) * n,
                          t == 0 ? nullptr : ego->rewards + (size_t)(t - 1) * n, 0))
      return 1;
    ph::RREnvStep es;
    std::memset(&es, 0, sizeof(es));
    es.stamps = rr_stamps(link, 0);
    es.want = want;
    es.timeout = link->timeout_cycles;
    es.error = link->error;
    es.joint = slot;
    es.partnerid = ego->partnerid;
    es.partner_trace = ego->partner_trace ? ego->partner_trace + (size_t)t * n : nullptr;
    es.base = ego->base_reward_seq + (size_t)t * n;
    es.done = ego->done_seq + (size_t)t * n;
    es.reward_out = ego->rewards + (size_t)t * n;
    es.alt_action_out = ego->alt_actions ? ego->alt_actions + (size_t)t * n : nullptr;
    es.next_block = ego->blocks + (size_t)((t + 1) % T) * n * ld;
    es.block_ld = ld;
    es.n_partners = K;
    es.n = n;
    es.bonus = ego->bonus;
    PH_HIP(ph::launch_rr_env_step(es, ctx->stream));
  }
  return 0;
}

int ph_roundrobin_partner_iteration(ph_ctx* ctx, const ph_rr_link* link, const ph_rr_partner* pa, int T,
                                    unsigned long long iteration) {
  DevGuard dev_guard(ctx);
  if (!ctx || !pa || T <= 0) return fail("ph_roundrobin_partner_iteration: bad argument");
  if (check_rr_link(link)) return 1;
  if (link->rank < 1) return fail("ph_roundrobin_partner_iteration: partners live on ranks 1 .. n_partners");
  if (!pa->params || !pa->es_scratch || !pa->can_scratch || !pa->pos || !pa->boundary || !pa->term ||
      !pa->open || !pa->prev_mask || !pa->actions || !pa->values || !pa->log_probs || !pa->rb)
    return fail("ph_roundrobin_partner_iteration: null argument");
  if (check_rb(pa->rb)) return 1;
  if (pa->rb->E != link->n) return fail("ph_roundrobin_partner_iteration: the rollout buffer must have one column per environment");
  const int n = link->n, k = link->rank - 1;
  for (int t = 0; t < T; ++t) {
    const unsigned long long want = iteration * (unsigned long long)T + (unsigned long long)t + 1ull;
    ph::RRPartnerStep st;
    std::memset(&st, 0, sizeof(st));
    st.block_stamp = rr_stamps(link, link->rank);
    st.act_stamp = rr_stamps(link, 0) + 1 + k;
    st.want = want;
    st.timeout = link->timeout_cycles;
    st.error = link->error;
    st.block = (const float*)rr_slot(link, link->rank, t & 1);
    st.block_ld = link->block_ld;
    st.n = n;
    st.T = pa->rb->T;
    st.k = k;
    st.rewards = pa->rb->rewards;
    st.pos = pa->pos;
    st.boundary = pa->boundary;
    st.term = pa->term;
    st.open = pa->open;
    st.prev_mask = pa->prev_mask;
    st.can = pa->can_scratch;
    st.es = pa->es_scratch;
    st.actions = pa->actions;
    st.act_dst = (int*)rr_slot(link, 0, t & 1) + (size_t)(1 + k) * n;
    PH_HIP(ph::launch_rr_partner_pre(st, ctx->stream));
    const float* obs_t = st.block + (size_t)n * 4;    // the observations follow the header rows in the slot
    if (ph_policy_forward_ragged(ctx, pa->spec, pa->params, obs_t, nullptr, pa->seed, pa->counter0 + (unsigned long long)t,
                                 0, pa->actions, pa->values, pa->log_probs, pa->rb, pa->pos, pa->can_scratch, pa->es_scratch))
      return 1;
    PH_HIP(ph::launch_rr_partner_post(st, ctx->stream));
  }
  return 0;
}

int ph_buffer_reset(ph_ctx* ctx, const ph_spec* spec, const ph_rollout* rb) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  ph_layout lay;
  if (layout_of(spec, &lay) || check_rb(rb)) return 1;
  const size_t n = (size_t)rb->T * rb->E;
  PH_HIP(hipMemsetAsync(rb->observations, 0, n * lay.D * sizeof(float), ctx->stream));
  PH_HIP(hipMemsetAsync(rb->actions, 0, n * lay.A * sizeof(float), ctx->stream));
  float* arrs[] = {rb->rewards, rb->episode_starts, rb->values, rb->log_probs, rb->advantages, rb->returns};
  for (float* a : arrs) PH_HIP(hipMemsetAsync(a, 0, n * sizeof(float), ctx->stream));
  return 0;
}

// ---- K2 ----
int ph_gae(ph_ctx* ctx, const ph_rollout* rb, const float* last_values, const float* dones, double gamma,
           double gae_lambda, int mode) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (check_rb(rb)) return 1;
  if (!last_values || !dones) return fail("ph_gae: null last_values/dones");
  if (mode < 0 || mode > 2) return fail("ph_gae: mode must be 0, 1 or 2");
  PH_HIP(ph::launch_gae(rb->rewards, rb->values, rb->episode_starts, last_values, dones, rb->advantages, rb->returns,
                        rb->T, rb->E, gamma, gae_lambda, mode, ctx->stream));
  return 0;
}

// ---- K4 ----
int ph_policy_forward(ph_ctx* ctx, const ph_spec* spec, const float* params, const float* obs, int n,
                      const unsigned char* action_mask, const float* uniforms, const float* given_actions,
                      unsigned long long seed, unsigned long long counter, int deterministic, int* actions_i32,
                      float* actions_f32, float* values, float* log_probs, float* entropy, float* logits,
                      const ph_rollout* rb, int pos, const float* episode_start_in, const float* pending_reward,
                      int gemm_mode) {
  DevGuard dev_guard(ctx);
  return forward_run("ph_policy_forward", ctx, spec, nullptr, params, obs, n, action_mask, uniforms, given_actions, seed, counter,
                     deterministic, actions_i32, actions_f32, values, log_probs, entropy, logits, rb, pos, episode_start_in,
                     pending_reward, gemm_mode);
}

int ph_policy_act_host(ph_ctx* ctx, const ph_spec* spec, const float* params, const float* obs_host, int n,
                       const float* episode_start_host, unsigned long long seed, unsigned long long counter, int deterministic,
                       int* actions_host, float* values_host, float* log_probs_host, const ph_rollout* rb, int pos, int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!params || !obs_host) return fail("ph_policy_act_host: null params/obs");
  if (n <= 0) return fail("ph_policy_act_host: n must be positive");
  if (rb && !episode_start_host) return fail("ph_policy_act_host: the fused rollout-buffer write needs episode_start_host");
  if (ctx->capturing) return fail("ph_policy_act_host synchronises: not inside graph capture");
  ph::NetDims nd;
  if (resolve(ctx, spec, &nd)) return 1;
  // staging layout (floats): obs n*D | episode_start n || actions n*A (as int32) | values n | log_probs n -- pinned, coherent host
  // memory the kernel reads and writes DIRECTLY (a few hundred bytes over the host link): no copy launches, one kernel, one wait
  const size_t n_in = (size_t)n * nd.D + (size_t)n, n_out = (size_t)n * nd.A + 2 * (size_t)n, need = n_in + n_out;
  if (need > ctx->act_stage_cap) {
    if (ctx->act_stage_host) (void)hipHostFree(ctx->act_stage_host);
    ctx->act_stage_host = nullptr;
    ctx->act_stage_dev = nullptr;
    ctx->act_stage_cap = 0;
    const size_t cap = need < 4096 ? 4096 : need;
    PH_HIP(hipHostMalloc((void**)&ctx->act_stage_host, cap * sizeof(float), hipHostMallocMapped | hipHostMallocCoherent));
    PH_HIP(hipHostGetDevicePointer((void**)&ctx->act_stage_dev, ctx->act_stage_host, 0));
    ctx->act_stage_cap = cap;
  }
  float *h = ctx->act_stage_host, *d = ctx->act_stage_dev;   // the same memory, host and device view
  std::memcpy(h, obs_host, (size_t)n * nd.D * sizeof(float));
  if (episode_start_host) std::memcpy(h + (size_t)n * nd.D, episode_start_host, (size_t)n * sizeof(float));
  else std::memset(h + (size_t)n * nd.D, 0, (size_t)n * sizeof(float));
  float* d_out = d + n_in;
  int* d_act = reinterpret_cast<int*>(d_out);
  float *d_val = d_out + (size_t)n * nd.A, *d_lp = d_val + n;
  // One tile of the 16-row forward = one policy and one value workgroup: each stores the launch's sequence number into its word
  // after its last output, and the host polls the two words (the outputs are in the same coherent memory, ordered before them).
  const bool words = n <= 16 && ph::fwd16_eligible(nd, n);
  if (words && !ctx->act_done_host) {
    PH_HIP(hipHostMalloc((void**)&ctx->act_done_host, 64, hipHostMallocMapped | hipHostMallocCoherent));
    PH_HIP(hipHostGetDevicePointer((void**)&ctx->act_done_dev, ctx->act_done_host, 0));
    ctx->act_done_host[0] = ctx->act_done_host[1] = 0;
  }
  if (words) {
    if (++ctx->act_seq == 0) ctx->act_seq = 1;
    ctx->fwd_host_done = ctx->act_done_dev;
  }
  const int frc = ph_policy_forward(ctx, spec, params, d, n, nullptr, nullptr, nullptr, seed, counter, deterministic, d_act,
                                    nullptr, d_val, d_lp, nullptr, nullptr, rb, pos, rb ? d + (size_t)n * nd.D : nullptr, nullptr,
                                    gemm_mode);
  ctx->fwd_host_done = nullptr;
  if (frc) return 1;
  bool arrived = false;
  if (words) {
    // a launch takes ~10 us end to end; a launch that has not signalled within 50 ms is waited for on the stream, which also
    // surfaces whatever error kept it from running
    const unsigned int seq = ctx->act_seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
      if (__atomic_load_n(ctx->act_done_host, __ATOMIC_ACQUIRE) == seq &&
          __atomic_load_n(ctx->act_done_host + 1, __ATOMIC_ACQUIRE) == seq) {
        arrived = true;
        break;
      }
      if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
      __builtin_ia32_pause();
    }
  }
  if (!arrived) PH_HIP(hipStreamSynchronize(ctx->stream));
  const float* h_out = h + n_in;
  if (actions_host) std::memcpy(actions_host, h_out, (size_t)n * nd.A * sizeof(int));
  if (values_host) std::memcpy(values_host, h_out + (size_t)n * nd.A, (size_t)n * sizeof(float));
  if (log_probs_host) std::memcpy(log_probs_host, h_out + (size_t)n * nd.A + n, (size_t)n * sizeof(float));
  return 0;
}

int ph_scripted_rollout(ph_ctx* ctx, const ph_spec* spec, const float* params, const float* obs_seq, const float* rew_seq,
                        const float* done_seq, int n, int n_steps, const float* episode_start0, unsigned long long seed,
                        unsigned long long counter0, int* actions_i32, float* values, float* log_probs, const ph_rollout* rb,
                        int pos0, int gemm_mode) {
  DevGuard dev_guard(ctx);
  return scripted_rollout_run("ph_scripted_rollout", ctx, spec, nullptr, params, obs_seq, rew_seq, done_seq, n, n_steps, episode_start0,
                              seed, counter0, actions_i32, values, log_probs, rb, pos0, gemm_mode);
}

namespace {
int step_multi_impl(ph_ctx* ctx, int n_calls, const ph_step_call* calls, const ph_p2p* x, int t);
int ensure_p2p_dev(ph_ctx* ctx, const ph_p2p* x);
}
int ph_policy_step_multi(ph_ctx* ctx, int n_calls, const ph_step_call* calls) {
  DevGuard dev_guard(ctx);
  return step_multi_impl(ctx, n_calls, calls, nullptr, 0);
}
namespace {
int step_multi_impl(ph_ctx* ctx, int n_calls, const ph_step_call* calls, const ph_p2p* x, int t) {
  if (!ctx) return fail("null ctx");
  if (!calls) return fail("ph_policy_step_multi: null calls");
  if (n_calls <= 0 || n_calls > ph::MAX_LOCAL_AGENTS) return fail("ph_policy_step_multi: 1..4 calls per launch");
  ph::FwdMulti m;
  std::memset(&m, 0, sizeof(m));
  for (int i = 0; i < n_calls; ++i) {
    const ph_step_call& c = calls[i];
    ph::FwdArgs& a = m.a[i];
    if (!c.params || !c.obs || !c.rb || !c.episode_start_in) return fail("ph_policy_step_multi: null argument");
    if ((uintptr_t)c.params % 16 != 0) return fail("ph_policy_step_multi: params must be 16-byte aligned");
    if (fwd_args(a, ctx, c.spec, false, c.params, c.obs, c.n, c.seed, c.counter, c.actions_i32, c.values, c.log_probs)) return 1;
    if (fwd_bind_row("ph_policy_step_multi", a, c.rb, c.pos, c.episode_start_in, c.pending_reward)) return 1;
    if (i > 0 && (c.n != calls[0].n || a.nd.Lp != m.a[0].nd.Lp))
      return fail("ph_policy_step_multi: all calls must share n and the padded logit count");
    a.mask = c.action_mask;
    a.deterministic = c.deterministic & 1;
    if (c.deterministic & (PH_STEP_FIX_ILLEGAL | PH_STEP_MASK_ENV_ONLY)) {
      if (!c.action_mask) return fail("PH_STEP_FIX_ILLEGAL / PH_STEP_MASK_ENV_ONLY need an action mask");
      if (!(a.nd.A == 1 && a.nd.L <= 8))
        return fail("PH_STEP_FIX_ILLEGAL: single Discrete head of at most 8 logits only (use ph_fix_illegal_actions)");
      a.env_mask = c.action_mask;
      if (c.deterministic & PH_STEP_MASK_ENV_ONLY) a.mask = nullptr;   // the policy never sees the mask (plain PPO partner)
    }
    if (c.pending_reward && c.joint_actions) {
      if (!c.partner_seat || c.n_seats <= 0 || c.seat < 0 || c.seat >= c.n_seats)
        return fail("ph_policy_step_multi: bad joint-action description");
      a.joint = c.joint_actions;
      a.n_seats = c.n_seats;
      a.seat = c.seat;
      a.partner_seat = c.partner_seat;
      a.bonus = c.bonus;
      a.reward_rule = ctx->joint_reward_rule;
    }
  }
  if (x) {  // exchange fused into the launch (16-row kernel only; the caller checked eligibility)
    if (!ph::fwd16_eligible(m.a[0].nd, m.a[0].n)) return fail("fused peer-to-peer step needs the 16-row forward kernel");
    if (x->count != n_calls * m.a[0].n) return fail("ph_p2p.count must be local agents x n");
    if (ensure_p2p_dev(ctx, x)) return 1;
    m.px.x = ctx->p2p_dev;
    m.px.t = t;
    m.px.a_local = n_calls;
    for (int i = 0; i < n_calls; ++i) {
      if (!m.a[i].joint) continue;   // consumers of the previous step's joint action read the stamp-in-band words
      const int prev = t >= 1 ? t - 1 : x->T - 1;   // step whose joint action this launch consumes (t = 0: last step of the previous iteration)
      m.a[i].joint_ll = x->ll[x->rank] + (size_t)(prev % x->ll_slots) * x->world * x->count;
      m.a[i].ll_epoch = x->epoch;
      m.a[i].ll_T = x->T;
      m.a[i].ll_t = t - 1;
      m.a[i].ll_timeout = x->timeout_cycles;
      m.a[i].ll_error = x->error;
    }
  }
  PH_HIP(ph::launch_policy_fwd_multi(m, n_calls, ctx->stream));
  return 0;
}
}  // namespace

// ---- RCCL exchange (librccl.so resolved at first use) ------------------------------------------------------------------
namespace {
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, ncclUniqueId, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
RcclApi* rccl_api() {
  static RcclApi api;
  static bool tried = false;
  if (!tried) {
    tried = true;
    for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
    }
    if (api.lib) {
      api.GetUniqueId = (int (*)(void*))dlsym(api.lib, "ncclGetUniqueId");
      api.CommInitRank = (int (*)(void**, int, ncclUniqueId, int))dlsym(api.lib, "ncclCommInitRank");
      api.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(api.lib, "ncclAllGather");
      api.CommDestroy = (int (*)(void*))dlsym(api.lib, "ncclCommDestroy");
      api.GetErrorString = (const char* (*)(int))dlsym(api.lib, "ncclGetErrorString");
      if (!api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.CommDestroy) api.lib = nullptr;
    }
  }
  return api.lib ? &api : nullptr;
}
int fail_rccl(const char* what, int rc) {
  RcclApi* r = rccl_api();
  std::string msg = std::string(what) + ": " + ((r && r->GetErrorString) ? r->GetErrorString(rc) : "RCCL error");
  return fail(msg.c_str());
}
}  // namespace

int ph_comm_unique_id(unsigned char* id_out) {
  if (!id_out) return fail("ph_comm_unique_id: null output");
  RcclApi* r = rccl_api();
  if (!r) return fail("ph_comm_unique_id: librccl.so could not be loaded");
  ncclUniqueId id;
  const int rc = r->GetUniqueId(&id);
  if (rc != 0) return fail_rccl("ncclGetUniqueId", rc);
  std::memcpy(id_out, id.internal, PH_COMM_ID_BYTES);
  return 0;
}

int ph_comm_init(ph_ctx* ctx, const unsigned char* id, int world, int rank) {
  DevGuard dev_guard(ctx);
  if (!ctx || !id) return fail("ph_comm_init: null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail("ph_comm_init: bad world / rank");
  if (ctx->comm) return fail("ph_comm_init: this context already has a communicator");
  RcclApi* r = rccl_api();
  if (!r) return fail("ph_comm_init: librccl.so could not be loaded");
  ncclUniqueId uid;
  std::memcpy(uid.internal, id, PH_COMM_ID_BYTES);
  void* comm = nullptr;
  const int rc = r->CommInitRank(&comm, world, uid, rank);
  if (rc != 0) return fail_rccl("ncclCommInitRank", rc);
  ctx->comm = comm;
  ctx->comm_world = world;
  ctx->comm_rank = rank;
  return 0;
}

int ph_comm_destroy(ph_ctx* ctx) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (ctx->comm) {
    RcclApi* r = rccl_api();
    if (r) (void)r->CommDestroy(ctx->comm);
    ctx->comm = nullptr;
    ctx->comm_world = 1;
    ctx->comm_rank = 0;
  }
  return 0;
}

int ph_all_gather_i32(ph_ctx* ctx, const int* local, int* joint, int count) {
  DevGuard dev_guard(ctx);
  if (!ctx || !local || !joint || count <= 0) return fail("ph_all_gather_i32: bad argument");
  if (!ctx->comm) {  // single process: the joint action is the local one
    PH_HIP(hipMemcpyAsync(joint, local, (size_t)count * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
  }
  RcclApi* r = rccl_api();
  const int rc = r->AllGather(local, joint, (size_t)count, (int)ncclInt32, ctx->comm, ctx->stream);
  if (rc != 0) return fail_rccl("ncclAllGather", rc);
  return 0;
}

int ph_selfplay_rollout(ph_ctx* ctx, int n_calls, const ph_step_call* calls, int T, const int* local, int* joint,
                        int count) {
  DevGuard dev_guard(ctx);
  if (!ctx || !calls || T <= 0) return fail("ph_selfplay_rollout: bad argument");
  for (int t = 0; t < T; ++t) {
    if (ph_policy_step_multi(ctx, n_calls, calls + (size_t)t * n_calls)) return 1;
    if (ph_all_gather_i32(ctx, local, joint, count)) return 1;
  }
  return 0;
}

// ---- peer-to-peer exchange buffers ---------------------------------------------------------------------------------------
int ph_p2p_alloc(ph_ctx* ctx, size_t bytes, void** ptr_out, unsigned char* handle_out) {
  DevGuard dev_guard(ctx);
  if (!ctx || !ptr_out || !handle_out || bytes == 0) return fail("ph_p2p_alloc: bad argument");
  void* p = nullptr;
  PH_HIP(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained));
  hipError_t e = hipMemset(p, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  hipIpcMemHandle_t hd;
  if (e == hipSuccess) e = hipIpcGetMemHandle(&hd, p);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return fail_hip("ph_p2p_alloc", e);
  }
  static_assert(sizeof(hd) == PH_IPC_HANDLE_BYTES, "IPC handle size");
  std::memcpy(handle_out, &hd, PH_IPC_HANDLE_BYTES);
  *ptr_out = p;
  return 0;
}
int ph_p2p_open(ph_ctx* ctx, const unsigned char* handle, void** ptr_out) {
  DevGuard dev_guard(ctx);
  if (!ctx || !handle || !ptr_out) return fail("ph_p2p_open: bad argument");
  hipIpcMemHandle_t hd;
  std::memcpy(&hd, handle, PH_IPC_HANDLE_BYTES);
  void* p = nullptr;
  PH_HIP(hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess));
  *ptr_out = p;
  return 0;
}
int ph_p2p_close(ph_ctx* ctx, void* ptr) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (ptr) PH_HIP(hipIpcCloseMemHandle(ptr));
  return 0;
}
int ph_p2p_free(ph_ctx* ctx, void* ptr) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (ptr) PH_HIP(hipFree(ptr));
  return 0;
}
namespace {
int check_p2p(const ph_p2p* x) {
  if (!x) return fail("null ph_p2p");
  if (x->world < 1 || x->world > PH_MAX_RANKS || x->rank < 0 || x->rank >= x->world || x->count <= 0 || x->T <= 0)
    return fail("ph_p2p: bad world / rank / count / T");
  if (!x->epoch || !x->error) return fail("ph_p2p: epoch and error words are required");
  for (int p = 0; p < x->world; ++p)
    if (!x->joint[0][p] || !x->joint[1][p] || !x->flags[p] || !x->ll[p]) return fail("ph_p2p: unmapped peer");
  if (x->ll_slots < x->T) return fail("ph_p2p: ll_slots must be >= T (a slot must not be reused inside an iteration)");
  return 0;
}
}  // namespace
int ph_p2p_push(ph_ctx* ctx, const ph_p2p* x, const int* local, int t) {
  DevGuard dev_guard(ctx);
  if (!ctx || !local) return fail("ph_p2p_push: null argument");
  if (check_p2p(x)) return 1;
  PH_HIP(ph::launch_p2p_push(*x, local, t, ctx->stream));
  return 0;
}
int ph_p2p_wait(ph_ctx* ctx, const ph_p2p* x, int t) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (check_p2p(x)) return 1;
  PH_HIP(ph::launch_p2p_wait(*x, t, ctx->stream));
  return 0;
}
int ph_p2p_ll_push(ph_ctx* ctx, const ph_p2p* x, const int* local, int t) {
  DevGuard dev_guard(ctx);
  if (!ctx || !local) return fail("ph_p2p_ll_push: null argument");
  if (check_p2p(x)) return 1;
  PH_HIP(ph::launch_p2p_ll_push(*x, local, t, ctx->stream));
  return 0;
}
int ph_p2p_ll_unpack(ph_ctx* ctx, const ph_p2p* x, int t) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (check_p2p(x)) return 1;
  PH_HIP(ph::launch_p2p_ll_unpack(*x, t, ctx->stream));
  return 0;
}
int ph_selfplay_rollout_p2p(ph_ctx* ctx, int n_calls, const ph_step_call* calls, int T, const int* local,
                            const ph_p2p* x) {
  DevGuard dev_guard(ctx);
  if (!ctx || !calls || !local || T <= 0) return fail("ph_selfplay_rollout_p2p: bad argument");
  if (check_p2p(x)) return 1;
  bool fused = x->count == n_calls * calls[0].n;
  for (int i = 0; i < n_calls && fused; ++i) {
    ph::NetDims nd;
    if (resolve(ctx, calls[i].spec, &nd)) return 1;
    fused = ph::fwd16_eligible(nd, calls[i].n);
  }
  if (fused) {
    // push and wait live inside the step launch; the stamp of the last step is awaited once, for whoever reads it next
    for (int t = 0; t < T; ++t)
      if (step_multi_impl(ctx, n_calls, calls + (size_t)t * n_calls, x, t)) return 1;
    PH_HIP(ph::launch_p2p_ll_unpack(*x, T - 1, ctx->stream));
    return 0;
  }
  for (int t = 0; t < T; ++t) {
    if (ph_policy_step_multi(ctx, n_calls, calls + (size_t)t * n_calls)) return 1;
    PH_HIP(ph::launch_p2p_push(*x, local, t, ctx->stream));
    PH_HIP(ph::launch_p2p_wait(*x, t, ctx->stream));
  }
  return 0;
}

namespace {
int ensure_p2p_dev(ph_ctx* ctx, const ph_p2p* x) {
  if (!ctx->p2p_dev) PH_HIP(hipMalloc((void**)&ctx->p2p_dev, sizeof(ph_p2p)));
  if (!ctx->p2p_valid || std::memcmp(&ctx->p2p_host, x, sizeof(ph_p2p)) != 0) {
    if (ctx->capturing) return fail("the peer-to-peer descriptor changed inside graph capture");
    ctx->p2p_host = *x;
    PH_HIP(hipMemcpyAsync(ctx->p2p_dev, &ctx->p2p_host, sizeof(ph_p2p), hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    ctx->p2p_valid = true;
  }
  return 0;
}
}  // namespace

int ph_selfplay_rollout_persistent_capacity(ph_ctx* ctx, int* workgroups_out) {
  DevGuard dev_guard(ctx);
  if (!ctx || !workgroups_out) return fail("ph_selfplay_rollout_persistent_capacity: null argument");
  if (ctx->exchange_blocks_per_cu <= 0) PH_HIP(ph::exchange_rollout_blocks_per_cu(&ctx->exchange_blocks_per_cu));
  *workgroups_out = ctx->exchange_blocks_per_cu * ctx->num_cu;
  return 0;
}

int ph_selfplay_rollout_persistent(ph_ctx* ctx, int n_calls, const ph_rollout_call* calls, int T, const ph_p2p* x,
                                   int ranks_on_device) {
  DevGuard dev_guard(ctx);
  if (!ctx || !calls || T <= 0) return fail("ph_selfplay_rollout_persistent: bad argument");
  if (n_calls <= 0 || n_calls > ph::MAX_LOCAL_AGENTS) return fail("ph_selfplay_rollout_persistent: 1..4 local agents");
  if (check_p2p(x)) return 1;
  if (x->T < T) return fail("ph_selfplay_rollout_persistent: ph_p2p.T must be >= the rollout length (stamps are epoch * x.T + t + 1)");
  if (x->ll_slots < 2 * x->T) return fail("ph_selfplay_rollout_persistent: ph_p2p.ll_slots must be >= 2 * ph_p2p.T (two alternating halves)");
  if (x->count != n_calls * calls[0].n) return fail("ph_p2p.count must be local agents x n");
  if (ranks_on_device < 1) ranks_on_device = 1;
  const long long wgs = (long long)n_calls * 2 * ((calls[0].n + 15) / 16) * ranks_on_device;
  int capacity = 0;
  if (ph_selfplay_rollout_persistent_capacity(ctx, &capacity)) return 1;
  if (wgs > (long long)capacity)
    return fail("ph_selfplay_rollout_persistent: the launch's workgroups would not all be resident (value workgroups poll): use "
                "ph_selfplay_rollout_p2p");
  ph::FwdMulti m;
  ph::ScriptedMulti sm;
  std::memset(&m, 0, sizeof(m));
  std::memset(&sm, 0, sizeof(sm));
  for (int i = 0; i < n_calls; ++i) {
    const ph_rollout_call& c = calls[i];
    ph::FwdArgs& a = m.a[i];
    if (!c.params || !c.obs_seq || !c.rew_seq || !c.done_seq || !c.rb || !c.episode_start0 || !c.partner_seat)
      return fail("ph_selfplay_rollout_persistent: null argument");
    if ((uintptr_t)c.params % 16 != 0) return fail("ph_selfplay_rollout_persistent: params must be 16-byte aligned");
    if (fwd_args(a, ctx, c.spec, false, c.params, c.obs_seq, c.n, c.seed, c.counter0, c.actions_i32, c.values, c.log_probs)) return 1;
    if (!ph::fwd16_eligible(a.nd, c.n))
      return fail("ph_selfplay_rollout_persistent: needs the 16-row forward's shape class (one feature chunk, one Discrete head "
                  "of <= 8 logits, n < 16384)");
    if (check_rb(c.rb)) return 1;
    if (c.n != c.rb->E || c.n != calls[0].n) return fail("ph_selfplay_rollout_persistent: every call's n must equal its rollout E and agree");
    if (c.rb->T < T) return fail("ph_selfplay_rollout_persistent: the rollout buffer has fewer than T rows");
    if (c.n_seats <= 0 || c.seat < 0 || c.seat >= c.n_seats) return fail("ph_selfplay_rollout_persistent: bad seat description");
    if (c.mask_mode < 0 || c.mask_mode > 3) return fail("ph_selfplay_rollout_persistent: mask_mode is 0..3");
    sm.sc[i].mask_policy = (c.mask_seq && (c.mask_mode == 0 || c.mask_mode == 1)) ? 1 : 0;
    sm.sc[i].mask_env = (c.mask_seq && (c.mask_mode == 1 || c.mask_mode == 2)) ? 1 : 0;
    a.mask = sm.sc[i].mask_policy ? c.mask_seq : nullptr;
    a.env_mask = sm.sc[i].mask_env ? c.mask_seq : nullptr;
    fwd_bind_bases(a, c.rb, c.episode_start0, nullptr, nullptr);
    a.joint = x->joint[0][x->rank];      // non-null marks "the reward has a joint-action term"; the kernel reads the words
    a.n_seats = c.n_seats;
    a.seat = c.seat;
    a.partner_seat = c.partner_seat;
    a.bonus = c.bonus;
    a.reward_rule = ctx->joint_reward_rule;
    a.ll_epoch = x->epoch;
    a.ll_T = x->T;
    a.ll_timeout = x->timeout_cycles;
    a.ll_error = x->error;
    sm.sc[i].n_steps = T;
    sm.sc[i].obs_seq = c.obs_seq;
    sm.sc[i].rew_seq = c.rew_seq;
    sm.sc[i].done_seq = c.done_seq;
    sm.sc[i].mask_seq = c.mask_seq;
  }
  if (ensure_p2p_dev(ctx, x)) return 1;
  m.px.x = ctx->p2p_dev;
  m.px.t = 0;
  m.px.a_local = n_calls;
  m.px.persistent = 1;
  PH_HIP(ph::launch_policy_fwd16_exchange_rollout(m, sm, n_calls, ctx->stream));
  // the last step's words -> the plain receive slot (ordinary consumers, route verification); waits for every peer once
  PH_HIP(ph::launch_p2p_ll_unpack(*x, T - 1, ctx->stream, -2));
  return 0;
}

int ph_policy_forward_ragged(ph_ctx* ctx, const ph_spec* spec, const float* params, const float* obs,
                             const unsigned char* action_mask, unsigned long long seed, unsigned long long counter,
                             int deterministic, int* actions_i32, float* values, float* log_probs, const ph_rollout* rb,
                             const int* pos_env, const unsigned char* record_mask, const float* episode_start_in) {
  DevGuard dev_guard(ctx);
  return forward_ragged_run("ph_policy_forward_ragged", ctx, spec, nullptr, params, obs, action_mask, seed, counter, deterministic,
                            actions_i32, values, log_probs, rb, pos_env, record_mask, episode_start_in, 0);   // gemm mode 0
}

int ph_buffer_add_reward_ragged(ph_ctx* ctx, const ph_rollout* rb, const int* pos_env, const float* reward,
                                const unsigned char* env_mask) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (check_rb(rb)) return 1;
  if (!pos_env || !reward) return fail("ph_buffer_add_reward_ragged: null argument");
  PH_HIP(ph::launch_reward_add_ragged(rb->rewards, pos_env, reward, env_mask, rb->T, rb->E, ctx->stream));
  return 0;
}

int ph_ragged_advance(ph_ctx* ctx, const ph_rollout* rb, int* pos_env, const unsigned char* record_mask) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (check_rb(rb)) return 1;
  if (!pos_env || !record_mask) return fail("ph_ragged_advance: null argument");
  PH_HIP(ph::launch_ragged_advance(pos_env, record_mask, rb->T, rb->E, ctx->stream));
  return 0;
}

int ph_fix_illegal_actions(ph_ctx* ctx, int* actions, const unsigned char* action_mask, int n, int L) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!actions || !action_mask) return fail("ph_fix_illegal_actions: null argument");
  if (n <= 0 || L <= 0) return fail("ph_fix_illegal_actions: bad sizes");
  PH_HIP(ph::launch_fix_illegal(actions, action_mask, n, L, ctx->stream));
  return 0;
}

// ---- vectorised game rules ----
int ph_rps_step(ph_ctx* ctx, const int* ego_actions, const int* alt_actions, float* ego_reward, float* alt_reward, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!ego_actions || !alt_actions || !ego_reward || !alt_reward) return fail("ph_rps_step: null argument");
  if (n <= 0) return fail("ph_rps_step: n must be positive");
  PH_HIP(ph::launch_rps_step(ego_actions, alt_actions, ego_reward, alt_reward, n, ctx->stream));
  return 0;
}

int ph_liar_step(ph_ctx* ctx, const int* hands, int* history, int* nmoves, const int* actions,
                 const unsigned char* is_ego, const unsigned char* active, float* obs_next, float* rewards,
                 unsigned char* done, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!hands || !history || !nmoves || !actions || !is_ego || !obs_next || !rewards || !done)
    return fail("ph_liar_step: null argument");
  if (n <= 0) return fail("ph_liar_step: n must be positive");
  if (((uintptr_t)hands | (uintptr_t)history) % 16 || ((uintptr_t)actions | (uintptr_t)obs_next | (uintptr_t)rewards) % 8)
    return fail(std::string("ph_liar_step") + LIAR_ALIGN16 + ", actions/obs_next/rewards 8-byte aligned");
  PH_HIP(ph::launch_liar_step(hands, history, nmoves, actions, is_ego, active, obs_next, rewards, done, n, ctx->stream));
  return 0;
}

int ph_liar_reset(ph_ctx* ctx, int* hands, int* history, int* nmoves, const unsigned char* reset_mask,
                  unsigned char* ego_first, unsigned long long seed, unsigned long long counter, float probegostart,
                  int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!hands || !history || !nmoves || !ego_first) return fail("ph_liar_reset: null argument");
  if (n <= 0) return fail("ph_liar_reset: n must be positive");
  if (((uintptr_t)hands | (uintptr_t)history) % 16) return fail_who("ph_liar_reset", LIAR_ALIGN16);
  PH_HIP(ph::launch_liar_reset(hands, history, nmoves, reset_mask, ego_first, seed, counter, ctx->rng_epoch, probegostart, n,
                               ctx->stream));
  return 0;
}

int ph_liar_obs(ph_ctx* ctx, const int* hands, const int* history, const int* nmoves, const unsigned char* is_ego,
                const unsigned char* active, float* obs_out, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!hands || !history || !nmoves || !is_ego || !obs_out) return fail("ph_liar_obs: null argument");
  if (n <= 0) return fail("ph_liar_obs: n must be positive");
  if (((uintptr_t)hands | (uintptr_t)history) % 16 || (uintptr_t)obs_out % 8)
    return fail(std::string("ph_liar_obs") + LIAR_ALIGN16 + ", obs_out 8-byte aligned");
  PH_HIP(ph::launch_liar_obs(hands, history, nmoves, is_ego, active, obs_out, n, ctx->stream));
  return 0;
}

namespace {
// One seat's forward inside a self-play step: the 64-wide kernels (arch == nullptr: exactly the calls the steps have always made)
// or the towers of a run-time shape.  Rectangular: recorded at row `pos` of rb.  Ragged: recorded at pos_env[e] where rec[e].
// A tower seat is always called with gemm_mode 0 although the per-call walk passes the policy's own mode.  The two agree only because
// the tower forward answers mode 1 with a VALU instantiation in the accumulation order of mode 0 and mode 2 with the mode-0 kernel
// itself, so every mode gives the bits of 0 (tests/test_gpu_arch_vec.py checks that for the ragged and the scripted calls).  A
// tower forward whose bits ever depend on the mode must take it from the step's description instead.
int seat_forward(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params, const float* obs, int n,
                 unsigned long long seed, unsigned long long counter, int* actions, float* values, float* log_probs,
                 const ph_rollout* rb, int pos, const float* episode_start) {
  return forward_run(arch ? "ph_arch_forward" : "ph_policy_forward", ctx, spec, arch, params, obs, n, nullptr, nullptr, nullptr, seed,
                     counter, 0, actions, nullptr, values, log_probs, nullptr, nullptr, rb, pos, episode_start, nullptr, 0);
}
int seat_forward_ragged(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params, const float* obs,
                        unsigned long long seed, unsigned long long counter, int* actions, float* values, float* log_probs,
                        const ph_rollout* rb, const int* pos_env, const unsigned char* rec, const float* episode_start) {
  return forward_ragged_run(arch ? "ph_arch_forward_ragged" : "ph_policy_forward_ragged", ctx, spec, arch, params, obs, nullptr, seed,
                            counter, 0, actions, values, log_probs, rb, pos_env, rec, episode_start, 0);
}

// The game block of a Liar's Dice step description (ph_liar_step.h's view of it) is complete, and what the kernels read in 16-byte
// and 8-byte vectors is aligned for it.  Host validation only: nothing is launched with a bad pointer.
int check_liar_game(const char* who, const ph::LiarGame& g) {
  if (g.n <= 0 || !g.hands || !g.history || !g.nmoves || !g.ego_first || !g.ego_actions || !g.alt_actions || !g.obs_ego || !g.obs_alt ||
      !g.obs_next || !g.rew1 || !g.rew2 || !g.done1 || !g.done2 || !g.running || !g.alt_opens || !g.ego_opens || !g.done)
    return fail_who(who, ": incomplete description");
  if (((uintptr_t)g.hands | (uintptr_t)g.history) % 16 ||
      ((uintptr_t)g.ego_actions | (uintptr_t)g.alt_actions | (uintptr_t)g.obs_ego | (uintptr_t)g.obs_alt | (uintptr_t)g.obs_next |
       (uintptr_t)g.rew1 | (uintptr_t)g.rew2) % 8)
    return fail(std::string(who) + LIAR_ALIGN16 + ", actions/observations/rewards 8-byte aligned");
  return 0;
}
extern "C++" {   // (templates below; the file's entry points are extern "C")
// ... and the ego of a training step has its rectangular buffer, one column per table
template <class Desc>
int check_liar_ego(const char* who, const Desc& s) {
  if (!s.spec || !s.ego_rb || !s.ego_params || !s.ego_episode_start || !s.episodes) return fail_who(who, ": incomplete description");
  if (check_rb(s.ego_rb)) return 1;
  if (s.ego_rb->E != s.n) return fail_who(who, ": buffers must have E = n");
  return 0;
}
template <class Desc>
ph::TrainEnd liar_train_end(const Desc& s, int ego_pos, int deal_only) {
  return ph::TrainEnd{deal_only ? nullptr : s.ego_rb->rewards + (size_t)ego_pos * s.n, s.ego_episode_start, s.episodes};
}
// the grouped forward runs the Liar's Dice 16-row one-hot class only
int check_liar_one_hot(const char* who, ph_ctx* ctx, const ph_spec* spec, int n) {
  ph::NetDims nd;
  if (resolve(ctx, spec, &nd)) return 1;
  if (!ph::pool_fwd_eligible(nd, n)) return fail_who(who, ": the spec is not the Liar's Dice 16-row one-hot class");
  return 0;
}

// a Liar's Dice self-play description is complete and its buffers hold one column per table
int check_liar_selfplay(const char* who, const ph_ctx* ctx, const ph_liar_selfplay* sp) {
  if (!ctx || !sp) return fail_who(who, ": null argument");
  const ph_liar_selfplay& s = *sp;
  if (check_liar_game(who, ph::liar_game_of(s))) return 1;
  if (!s.alt_rb || !s.alt_params || !s.alt_pos || !s.alt_boundary || !s.alt_term || !s.alt_open || !s.alt_acted || !s.can || !s.es_alt)
    return fail_who(who, ": incomplete description");
  if (check_liar_ego(who, s) || check_rb(s.alt_rb)) return 1;
  if (s.alt_rb->E != s.n) return fail_who(who, ": buffers must have E = n");
  return 0;
}

// The launch sequence of one vectorised Liar's Dice step, written once (ph_liar_step.h):
//   seat-0 forward | after_ego | seat-1 forward (reply) | after_reply | seat-1 forward (openers) | after_opening
// and its re-deal half alone (deal_only: for the tables flagged in g.done).  seat0() and seat1(obs, active, counter) run a
// seat's forward; k = the Philox counters of the three forwards; the dice (and the pool's resample) draw with `counter`.
// With a recorder attached (ph_liar_record_attach) the two record launches of ph_record.h stand where the scratch they read
// is still intact: behind the reply forward, and behind the opening forward.  `seats`: who sits where, for the log's member column.
struct LiarSeats {
  const int *ego_id, *alt_id;        // (n) member at seat 0 / seat 1, or null: member 0
  const unsigned char* playing;      // (n) the tables that take part, or null: all
};
struct NoRedraw {   // ended(deal_only): what follows the pass that ends games, before seat 1 opens the new ones (ADAP redraws there)
  int operator()(int) const { return 0; }
};
template <class Book, class End, class Seat0, class Seat1, class Ended = NoRedraw>
int liar_step_run(ph_ctx* ctx, const ph::LiarGame& g, const Book& book, const End& end, unsigned long long counter, int deal_only,
                  const unsigned long long (&k)[3], const LiarSeats& seats, Seat0 seat0, Seat1 seat1, Ended ended = Ended{}) {
  hipStream_t st = ctx->stream;
  const bool rec = ctx->recording;
  if (rec && ctx->rec.n != g.n)
    return fail("Liar's Dice step: the attached recorder holds " + std::to_string(ctx->rec.n) + " tables, the step " +
                std::to_string(g.n) + " (ph_liar_record_attach)");
  const ph::RecordStep rs{g.obs_ego, g.obs_alt, g.obs_next, g.ego_actions, g.alt_actions, g.done1, g.done2,
                          g.running, g.alt_opens, seats.ego_id, seats.alt_id, seats.playing};
  if (!deal_only) {
    if (seat0(k[0])) return 1;                               // seat 0 moves in every table
    PH_HIP(ph::launch_liar_pass(0, g, book, end, counter, ctx->rng_epoch, deal_only, st));
    if (seat1(g.obs_next, g.running, k[1])) return 1;        // seat 1 replies where the game goes on (obs_next = its observation there)
    if (rec) PH_HIP(ph::launch_record_moves(ctx->rec, rs, st));
  }
  // reply played and credited; finished tables are re-dealt; where seat 1 opens the new game it moves once
  PH_HIP(ph::launch_liar_pass(1, g, book, end, counter, ctx->rng_epoch, deal_only, st));
  if (ended(deal_only)) return 1;
  if (seat1(g.obs_alt, g.alt_opens, k[2])) return 1;
  if (rec) PH_HIP(ph::launch_record_opening(ctx->rec, rs, st));
  PH_HIP(ph::launch_liar_pass(2, g, book, end, counter, ctx->rng_epoch, deal_only, st));
  return 0;
}

}  // extern "C++"

// ---- ADAP seats (ph_adap_vec.h) ----
// the row shape of an environment space under a context of C floats; host validation only
int adap_row_shape(const char* who, const ph_space* env, int C, ph::AdapRowShape* out) {
  if (!env) return fail_who(who, ": null observation space");
  if (C < 1 || C > ph::ADAP_VEC_MAX_CONTEXT)
    return fail(std::string(who) + ": context_size must be 1.." + std::to_string(ph::ADAP_VEC_MAX_CONTEXT));
  std::memset(out, 0, sizeof(*out));
  out->C = C;
  if (env->kind == PH_SPACE_BOX) {
    if (env->n < 1) return fail_who(who, ": an empty Box observation");
    out->box = 1;
    out->D = out->F = env->n;
    return 0;
  }
  if (env->kind != PH_SPACE_DISCRETE) return fail_who(who, ": the observation space must be a Box or of the Discrete family");
  if (env->n < 1 || env->n > PH_MAX_COMP) return fail_who(who, ": the observation space holds 1..PH_MAX_COMP components");
  out->D = env->n;
  for (int i = 0; i < env->n; ++i) {
    if (env->nvec[i] < 1) return fail_who(who, ": a component of the observation space has no category");
    out->off[i + 1] = out->off[i] + env->nvec[i];
  }
  out->F = out->off[env->n];
  return 0;
}
int check_adap_sampler(const char* who, int sampler, int C) {
  if (sampler < PH_CTX_L2 || sampler > PH_CTX_NATURAL_NUMBERS) return fail_who(who, ": unknown context sampler");
  if (sampler == PH_CTX_NATURAL_NUMBERS && C != 1)
    return fail_who(who, ": PH_CTX_NATURAL_NUMBERS draws one integer: it needs context_size == 1 (adap/util.py:80-89)");
  return 0;
}

// the Liar's Dice observation an ADAP seat's rows are built from: MultiDiscrete([7] * 6 + [7, 12] * 12), 30 components, 270 features
void liar_env_space(ph_space* env) {
  std::memset(env, 0, sizeof(*env));
  env->kind = PH_SPACE_DISCRETE;
  env->n = 6 + 2 * ph::LD_MAXMOVES;
  for (int i = 0; i < env->n; ++i) env->nvec[i] = (i < 6 || (i - 6) % 2 == 0) ? ph::LD_SIDES + 1 : 2 * ph::LD_DICE;
}

// an ADAP seat of a Liar's Dice step is well formed: a Box(F + C) spec, a sampler that takes C, its planes, aligned parameters
int check_adap_seat(const char* who, const char* seat, const ph_adap_seat* a, const ph_adap_seat* other, const float* params,
                    ph::AdapRowShape* shape) {
  const std::string w = std::string(who) + ": " + seat + " seat";
  if (!a->spec) return fail(w + ": null spec");
  ph_space env;
  liar_env_space(&env);
  if (adap_row_shape(w.c_str(), &env, a->context_size, shape)) return 1;
  if (check_adap_sampler(w.c_str(), a->sampler, a->context_size)) return 1;
  if (a->spec->obs.kind != PH_SPACE_BOX || a->spec->obs.n != shape->F + shape->C)
    return fail(w + ": the spec's observation must be a Box of F + C = " + std::to_string(shape->F + shape->C) + " components");
  if (!a->rows) return fail(w + ": null rows");
  if (a->shared) {
    if (!other || other->shared || !other->contexts) return fail(w + ": shared != 0 needs an ADAP seat that draws on the other side");
    if (other->context_size != a->context_size) return fail(w + ": shared != 0 needs the other seat's context_size");
  } else if (!a->contexts) {
    return fail(w + ": null contexts");
  }
  if (((uintptr_t)a->rows | (uintptr_t)a->contexts) % 4 || (uintptr_t)params % 16)
    return fail(w + ": rows/contexts must be 4-byte aligned, params 16-byte aligned");
  return 0;
}

// self-play: either seat on the 64-wide kernels (null arch) or on towers, or an ADAP learner (its rows built in front of its forward,
// its contexts redrawn behind the pass that ends games); the partner's forwards are ragged
int liar_selfplay_step_run(const char* who, ph_ctx* ctx, const ph_liar_selfplay* sp, const ph_arch* ego_arch, const ph_arch* alt_arch,
                           int ego_pos, unsigned long long counter, int deal_only, const ph_adap_seat* ego_adap = nullptr,
                           const ph_adap_seat* alt_adap = nullptr) {
  if (check_liar_selfplay(who, ctx, sp)) return 1;
  const ph_liar_selfplay& s = *sp;
  if (!deal_only && (ego_pos < 0 || ego_pos >= s.ego_rb->T)) return fail_who(who, ": ego_pos out of range (buffer full?)");
  ph::AdapRowShape ego_shape, alt_shape;
  if (ego_adap && check_adap_seat(who, "ego", ego_adap, alt_adap, s.ego_params, &ego_shape)) return 1;
  if (alt_adap && check_adap_seat(who, "partner", alt_adap, ego_adap, s.alt_params, &alt_shape)) return 1;
  const float* ego_ctx = ego_adap ? (ego_adap->shared ? alt_adap->contexts : ego_adap->contexts) : nullptr;
  const float* alt_ctx = alt_adap ? (alt_adap->shared ? ego_adap->contexts : alt_adap->contexts) : nullptr;
  hipStream_t st = ctx->stream;
  const ph::LearnerBook book{ph::SeatFields{s.n, s.alt_pos, s.alt_boundary, s.alt_term, s.alt_open, s.alt_acted, s.can, s.es_alt},
                             s.alt_rb->rewards, s.alt_rb->T};
  return liar_step_run(
      ctx, ph::liar_game_of(s), book, liar_train_end(s, ego_pos, deal_only), counter, deal_only, {counter, 2 * counter, 2 * counter + 1},
      LiarSeats{nullptr, nullptr, nullptr},
      [&](unsigned long long c) {
        const float* obs = s.obs_ego;
        if (ego_adap) {
          PH_HIP(ph::launch_adap_rows(ego_shape, s.obs_ego, ego_ctx, nullptr, ego_adap->rows, s.n, st));
          obs = ego_adap->rows;
        }
        return seat_forward(ctx, ego_adap ? ego_adap->spec : s.spec, ego_arch, s.ego_params, obs, s.n, s.ego_seed, c, s.ego_actions,
                            s.ego_values, s.ego_log_probs, s.ego_rb, ego_pos, s.ego_episode_start);
      },
      [&](const float* obs, const unsigned char* active, unsigned long long c) {
        if (alt_adap) {
          PH_HIP(ph::launch_adap_rows(alt_shape, obs, alt_ctx, active, alt_adap->rows, s.n, st));
          obs = alt_adap->rows;
        }
        return seat_forward_ragged(ctx, alt_adap ? alt_adap->spec : s.spec, alt_arch, s.alt_params, obs, s.alt_seed, c, s.alt_actions,
                                   s.alt_values, s.alt_log_probs, s.alt_rb, s.alt_pos, s.can, s.es_alt);
      },
      [&](int deal) {   // both seats were paid `done` in the tables whose game just ended (pantheon_hip.h: a game never ends on its opening move)
        if (deal) return 0;   // the first contexts of a run are the caller's
        for (const ph_adap_seat* a : {ego_adap, alt_adap})
          if (a && !a->shared)
            PH_HIP(ph::launch_adap_context_draw(a->sampler, a->context_size, a->seed, counter, ctx->rng_epoch, s.done, a->contexts, s.n,
                                                st));
        return 0;
      });
}
}  // namespace

int ph_liar_selfplay_step(ph_ctx* ctx, const ph_liar_selfplay* sp, int ego_pos, unsigned long long counter, int deal_only) {
  DevGuard dev_guard(ctx);
  return liar_selfplay_step_run("ph_liar_selfplay_step", ctx, sp, nullptr, nullptr, ego_pos, counter, deal_only);
}

int ph_liar_selfplay_step_arch(ph_ctx* ctx, const ph_liar_selfplay* sp, const ph_arch* ego_arch, const ph_arch* alt_arch, int ego_pos,
                               unsigned long long counter, int deal_only) {
  DevGuard dev_guard(ctx);
  return liar_selfplay_step_run("ph_liar_selfplay_step_arch", ctx, sp, ego_arch, alt_arch, ego_pos, counter, deal_only);
}

int ph_liar_selfplay_step_adap(ph_ctx* ctx, const ph_liar_selfplay* sp, const ph_adap_seat* ego, const ph_adap_seat* alt, int ego_pos,
                               unsigned long long counter, int deal_only) {
  DevGuard dev_guard(ctx);
  return liar_selfplay_step_run("ph_liar_selfplay_step_adap", ctx, sp, nullptr, nullptr, ego_pos, counter, deal_only, ego, alt);
}

int ph_adap_rows(ph_ctx* ctx, const ph_space* env_obs_space, int context_size, const float* obs, const float* contexts,
                 const unsigned char* active, float* rows, int n) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_adap_rows";
  if (!ctx) return fail("null ctx");
  ph::AdapRowShape shape;
  if (adap_row_shape(who, env_obs_space, context_size, &shape)) return 1;
  if (!obs || !contexts || !rows) return fail_who(who, ": null argument");
  if (n <= 0 || (long long)n * (shape.F + shape.C) >= (1ll << 31)) return fail_who(who, ": n must be positive and n * (F + C) fit in int32");
  if (((uintptr_t)obs | (uintptr_t)contexts | (uintptr_t)rows) % 4) return fail_who(who, ": obs/contexts/rows must be 4-byte aligned");
  PH_HIP(ph::launch_adap_rows(shape, obs, contexts, active, rows, n, ctx->stream));
  return 0;
}

int ph_adap_context_draw(ph_ctx* ctx, int sampler, int context_size, unsigned long long seed, unsigned long long counter,
                         const unsigned char* redraw, float* contexts, int n) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_adap_context_draw";
  if (!ctx) return fail("null ctx");
  if (context_size < 1 || context_size > ph::ADAP_VEC_MAX_CONTEXT)
    return fail(std::string(who) + ": context_size must be 1.." + std::to_string(ph::ADAP_VEC_MAX_CONTEXT));
  if (check_adap_sampler(who, sampler, context_size)) return 1;
  if (!contexts || (uintptr_t)contexts % 4) return fail_who(who, ": contexts must be a 4-byte aligned array");
  if (n <= 0) return fail_who(who, ": n must be positive");
  PH_HIP(ph::launch_adap_context_draw(sampler, context_size, seed, counter, ctx->rng_epoch, redraw, contexts, n, ctx->stream));
  return 0;
}

int ph_adap_vec_host(const ph_space* env_obs_space, int context_size, int sampler, int do_draw, unsigned long long seed,
                     unsigned long long counter, const unsigned char* redraw, float* contexts, const float* obs,
                     const unsigned char* active, float* rows, int n) {
  const char* who = "ph_adap_vec_host";
  if (n <= 0 || !contexts) return fail_who(who, ": n must be positive and contexts given");
  if (context_size < 1 || context_size > ph::ADAP_VEC_MAX_CONTEXT)
    return fail(std::string(who) + ": context_size must be 1.." + std::to_string(ph::ADAP_VEC_MAX_CONTEXT));
  if (do_draw) {
    if (check_adap_sampler(who, sampler, context_size)) return 1;
    for (int e = 0; e < n; ++e)
      if (!redraw || redraw[e])
        ph::adap_draw_context(sampler, context_size, seed, ph::adap_vec_counter(counter, nullptr), (uint32_t)e,
                              contexts + (size_t)e * context_size);
  }
  if (!rows) return 0;
  ph::AdapRowShape shape;
  if (adap_row_shape(who, env_obs_space, context_size, &shape)) return 1;
  if (!obs) return fail_who(who, ": rows need obs");
  const int W = shape.F + shape.C;
  for (int e = 0; e < n; ++e) {
    if (active && !active[e]) continue;
    for (int f = 0; f < W; ++f)
      rows[(size_t)e * W + f] =
          ph::adap_row_value(shape, shape.off, obs + (size_t)e * shape.D, contexts + (size_t)e * context_size, f);
  }
  return 0;
}

// ---- Liar's Dice against a pool of partners (ph_pool.h) ----
namespace {
// an ADAP member of the Liar's Dice pool is well formed: C in range, its contexts, a sampler that takes C, a Box(270 + C) spec with
// the step's heads; its parameter layout goes to *lay
int check_pool_adap(const char* who, const ph_spec* spec, const ph_pool_adap& ap, ph_layout* lay) {
  const std::string w(who);
  ph_space env;
  liar_env_space(&env);
  ph::AdapRowShape shape;
  if (adap_row_shape(who, &env, ap.context_size, &shape)) return 1;
  if (!ap.contexts) return fail(w + ": null contexts");
  if ((uintptr_t)ap.contexts % 4) return fail(w + ": contexts must be 4-byte aligned");
  if (check_adap_sampler(who, ap.sampler, ap.context_size)) return 1;
  if (!ap.spec) return fail(w + ": null ADAP spec");
  if (ap.spec->obs.kind != PH_SPACE_BOX || ap.spec->obs.n != shape.F + shape.C)
    return fail(w + ": the ADAP spec's observation must be a Box of 270 + C = " + std::to_string(shape.F + shape.C) + " components");
  if (ap.spec->act.kind != spec->act.kind || ap.spec->act.n != spec->act.n ||
      std::memcmp(ap.spec->act.nvec, spec->act.nvec, sizeof(int) * (size_t)(spec->act.n > 0 ? spec->act.n : 0)) != 0)
    return fail(w + ": the ADAP spec's action space must be the step's (Liar's Dice: (A, L) = (2, 19))");
  if (layout_of(ap.spec, lay)) return 1;
  if (lay->A != 2 || lay->L != 19) return fail(w + ": the ADAP spec's heads must be Liar's Dice's (A, L) = (2, 19)");
  return 0;
}

// validate the members and bring the device-side table up to date (uploaded only when it changed; never inside graph capture).
// archs: null, or per member null (the member stays what its kind says on the 64-wide / scripted / clone kernels) or the arch of a
// learner's or frozen member's towers, resolved into the table for pool_tower_kernel.  adaps: null, or per member null or the
// description of the AdapPolicy checkpoint a frozen member plays (pool_adap_kernel's tiles).
int pool_members(ph_ctx* ctx, const char* who, const ph_spec* spec, const ph_pool_member* members, const ph_arch* const* archs,
                 const ph_pool_adap* const* adaps, int K, int n) {
  const std::string w(who);
  if (!members) return fail(w + ": null member array");
  if (K < 1 || K > PH_MAX_POOL) return fail(w + ": the pool holds 1..PH_MAX_POOL members");
  if ((archs || adaps) && !spec) return fail(w + ": null spec");
  ph::PoolMemberDev tab[PH_MAX_POOL];
  // (the K rows in use are zeroed, compared and uploaded: this runs in front of every step)
  const size_t used = sizeof(ph::PoolMemberDev) * (size_t)K;
  std::memset(tab, 0, used);
  bool wide = false, adap = false;
  size_t tower_lds = 0;
  for (int k = 0; k < K; ++k) {
    const ph_pool_member& m = members[k];
    ph::PoolMemberDev& d = tab[k];
    const std::string wk = w + ": member " + std::to_string(k);
    if (m.kind != PH_POOL_LEARNER && m.kind != PH_POOL_FROZEN && m.kind != PH_POOL_SCRIPTED && m.kind != PH_POOL_CLONE)
      return fail(wk + ": unknown kind");
    d.kind = d.fwd = m.kind;
    if (adaps && adaps[k]) {
      const ph_pool_adap& ap = *adaps[k];
      if (m.kind != PH_POOL_FROZEN) return fail(wk + ": an ADAP checkpoint is a PH_POOL_FROZEN member (ADAP learners do not sit in a pool)");
      if (archs && archs[k]) return fail(wk + ": an ADAP member takes no arch");
      if (check_pool_adap(wk.c_str(), spec, ap, &d.adap_lay)) return 1;
      d.adap_C = ap.context_size;
      d.adap_ctx = ap.contexts;
      d.fwd = PH_POOL_CLONE;   // "not pool_fwd16h_kernel's tile"
      adap = true;
    } else if (archs && archs[k]) {
      if (m.kind == PH_POOL_SCRIPTED || m.kind == PH_POOL_CLONE)
        return fail(wk + ": an arch belongs to a learner or a frozen member, not to a scripted one or a clone");
      ph::NetDims nd;
      ph::ArchDims ad;
      if (arch_host_dims(spec, archs[k], &nd, &ad) || arch_lds_refusal(nd, ad)) return 1;
      d.ad = ad;
      d.fwd = PH_POOL_CLONE;   // "not pool_fwd16h_kernel's tile"
      d.tower = 1;
      tower_lds = std::max(tower_lds, ph::arch_fwd_lds_bytes(nd, ad));   // (nd: the fields the carve depends on)
    } else if (m.kind != PH_POOL_CLONE) {
      wide = true;
    }
    if (m.kind == PH_POOL_SCRIPTED) continue;
    if (!m.params) return fail(wk + ": null params");
    if ((uintptr_t)m.params % 16 != 0) return fail(wk + ": params must be 16-byte aligned");
    d.params = m.params;
    d.seed = m.seed;
    if (m.kind == PH_POOL_CLONE) continue;   // a ph_bc_layout vector and its key: every other field is ignored
    d.values = m.values;
    d.log_probs = m.log_probs;
    if (m.kind == PH_POOL_FROZEN) continue;
    if (!m.rb) return fail(wk + ": a learner needs its rollout buffer");
    if (check_rb(m.rb)) return 1;
    if (m.rb->E != n) return fail(wk + ": the learner's buffer must have E = n");
    if (!m.pos || !m.boundary || !m.term || !m.open || !m.values || !m.log_probs)
      return fail(wk + ": a learner needs pos / boundary / term / open / values / log_probs");
    d.rb_T = m.rb->T;
    d.rb_obs = m.rb->observations;
    d.rb_act = m.rb->actions;
    d.rb_rew = m.rb->rewards;
    d.rb_es = m.rb->episode_starts;
    d.rb_val = m.rb->values;
    d.rb_logp = m.rb->log_probs;
    d.pos = m.pos;
    d.boundary = m.boundary;
    d.term = m.term;
    d.open = m.open;
  }
  if (ctx->pool_count != K || std::memcmp(ctx->pool_host, tab, used) != 0) {
    if (ctx->capturing) return fail(w + ": the member table changed inside graph capture: run the same call once outside capture first");
    if (!ctx->pool_dev) PH_HIP(hipMalloc((void**)&ctx->pool_dev, sizeof(tab)));
    PH_HIP(hipStreamSynchronize(ctx->stream));   // launches in flight still read the table
    std::memcpy(ctx->pool_host, tab, used);
    ctx->pool_count = 0;
    PH_HIP(hipMemcpyAsync(ctx->pool_dev, ctx->pool_host, used, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    ctx->pool_count = K;
    ctx->pool_wide = wide;
    ctx->pool_tower_lds = tower_lds;
    ctx->pool_adap = adap;
  }
  return 0;
}

// one redraw launch per sampling ADAP member, behind the pass that ends games: the tables that pass has just dealt (alt_opens or
// ego_opens: every table whose game ended and that plays on -- in the pool that is `done`; a retired table of an evaluation keeps a
// stale `done` -- and, in a deal-only call, the tables the caller flagged) get a new context of that member, drawn at the step's
// counter under the member's seed
int pool_adap_redraw(ph_ctx* ctx, const ph_pool_member* members, const ph_pool_adap* const* adaps, int K, unsigned long long counter,
                     const ph::LiarGame& g) {
  if (!adaps) return 0;
  for (int k = 0; k < K; ++k)
    if (adaps[k] && adaps[k]->draw)
      PH_HIP(ph::launch_adap_context_draw(adaps[k]->sampler, adaps[k]->context_size, members[k].seed, counter, ctx->rng_epoch, g.alt_opens,
                                          adaps[k]->contexts, g.n, ctx->stream, g.ego_opens));
  return 0;
}

// the shared-trunk layout of the spec when the context's member table holds a clone (checked against the clone tile), else P = 0
int pool_clone_layout(const char* who, ph_ctx* ctx, const ph_spec* spec, const ph::NetDims& nd, ph_bc_layout* out) {
  std::memset(out, 0, sizeof(*out));
  bool clone = false;
  for (int k = 0; k < ctx->pool_count; ++k) clone = clone || ctx->pool_host[k].kind == PH_POOL_CLONE;
  if (!clone) return 0;
  if (ph_bc_layout_of(spec, out)) return 1;
  if (!ph::pool_clone_eligible(nd, *out))
    return fail(std::string(who) + ": a PH_POOL_CLONE member needs one-hot observations of at most 32 components and at most 32 logits");
  return 0;
}
// the same check in front of a step's first launch
int check_pool_clones(const char* who, ph_ctx* ctx, const ph_spec* spec) {
  ph::NetDims nd;
  ph_bc_layout lay;
  if (resolve(ctx, spec, &nd)) return 1;
  return pool_clone_layout(who, ctx, spec, nd, &lay);
}

// bucket pass + the grouped forward over the tables with active[e] != 0
int pool_forward(ph_ctx* ctx, const char* who, const ph_spec* spec, int K, const float* obs, const int* partnerid,
                 const unsigned char* active, const unsigned char* rec_mask, unsigned long long counter, int* actions,
                 const float* es_in, int n) {
  ph::PoolFwd p;
  std::memset(&p, 0, sizeof(p));
  if (fwd_args(p.a, ctx, spec, false, nullptr, obs, n, 0, counter, actions, nullptr, nullptr)) return 1;
  if (!ph::pool_fwd_eligible(p.a.nd, n))
    return fail(std::string(who) + ": the spec is not the Liar's Dice 16-row one-hot class (30 observation components, <= 32 logits, "
                                   "two action components, n < 16384)");
  if (pool_clone_layout(who, ctx, spec, p.a.nd, &p.bc)) return 1;
  p.a.rec_mask = rec_mask;
  p.a.es_in = es_in;
  if (ensure(ctx, ctx->pool_order, ctx->pool_order_cap, (size_t)n)) return 1;
  const size_t ntile = (size_t)ph::pool_max_tiles(n, PH_MAX_POOL);
  if (ensure(ctx, ctx->pool_tiles, ctx->pool_tiles_cap, 3 * (ntile + 1))) return 1;
  p.members = ctx->pool_dev;
  p.b.order = ctx->pool_order;
  p.b.tiles = ctx->pool_tiles;
  p.b.ntiles = ctx->pool_tiles + 3 * ntile;
  PH_HIP(ph::launch_pool_bucket(partnerid, active, n, K, p.b, ctx->stream));
  // which of the three kernels the table has tiles for (pool_members found out at the upload): 64-wide and scripted members,
  // clones (p.bc.P), towers (their largest carve), ADAP members
  PH_HIP(ph::launch_pool_fwd(p, K, ctx->stream, !ctx->pool_wide, ctx->pool_tower_lds, ctx->pool_adap));
  return 0;
}
}  // namespace

int ph_pool_forward(ph_ctx* ctx, const ph_spec* spec, const ph_pool_member* members, int n_members, const float* obs,
                    const int* partnerid, const unsigned char* active, unsigned long long counter, int* actions,
                    const float* episode_start_in, int n) {
  return ph_pool_forward_arch(ctx, spec, members, n_members, obs, partnerid, active, counter, actions, episode_start_in, n, nullptr);
}

int ph_pool_forward_arch(ph_ctx* ctx, const ph_spec* spec, const ph_pool_member* members, int n_members, const float* obs,
                         const int* partnerid, const unsigned char* active, unsigned long long counter, int* actions,
                         const float* episode_start_in, int n, const ph_arch* const* member_archs) {
  return ph_pool_forward_adap(ctx, spec, members, n_members, obs, partnerid, active, counter, actions, episode_start_in, n, member_archs,
                              nullptr);
}

int ph_pool_forward_adap(ph_ctx* ctx, const ph_spec* spec, const ph_pool_member* members, int n_members, const float* obs,
                         const int* partnerid, const unsigned char* active, unsigned long long counter, int* actions,
                         const float* episode_start_in, int n, const ph_arch* const* member_archs,
                         const ph_pool_adap* const* member_adaps) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!spec || !obs || !partnerid || !active || !actions) return fail("ph_pool_forward: null argument");
  if (n <= 0) return fail("ph_pool_forward: n must be positive");
  if ((uintptr_t)actions % 8) return fail("ph_pool_forward: actions must be 8-byte aligned");
  if (pool_members(ctx, "ph_pool_forward", spec, members, member_archs, member_adaps, n_members, n) ||
      check_pool_clones("ph_pool_forward", ctx, spec))
    return 1;
  for (int k = 0; k < n_members; ++k)
    if (members[k].kind == PH_POOL_LEARNER && !episode_start_in) return fail("ph_pool_forward: learners need episode_start_in");
  return pool_forward(ctx, "ph_pool_forward", spec, n_members, obs, partnerid, active, active, counter, actions, episode_start_in, n);
}

int ph_liar_default_actions(ph_ctx* ctx, const float* obs, const unsigned char* active, int* actions, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!obs || !actions) return fail("ph_liar_default_actions: null argument");
  if (n <= 0) return fail("ph_liar_default_actions: n must be positive");
  if ((uintptr_t)actions % 8) return fail("ph_liar_default_actions: actions must be 8-byte aligned");
  PH_HIP(ph::launch_liar_default_actions(obs, active, actions, n, ctx->stream));
  return 0;
}

// The pool step and the cross-play step, each written once for the entry point and its `_arch` form: C++ overloads of the entry
// points' names that take the archs and the ADAP descriptions as well (null: every seat on today's kernels).
extern "C++" {
namespace {
int ph_liar_pool_step(ph_ctx* ctx, const ph_liar_pool* pool, const ph_arch* ego_arch, const ph_arch* const* member_archs,
                      const ph_pool_adap* const* member_adaps, int ego_pos, unsigned long long counter, int deal_only) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_liar_pool_step";
  if (!ctx || !pool) return fail_who(who, ": null argument");
  const ph_liar_pool& s = *pool;
  const ph::LiarGame g = ph::liar_game_of(s);
  if (check_liar_game(who, g)) return 1;
  if (!s.partnerid || !s.alt_acted || !s.can || !s.es_alt) return fail_who(who, ": incomplete description");
  if (s.resample != PH_POOL_ROBIN && s.resample != PH_POOL_RANDOM) return fail_who(who, ": unknown resample rule");
  if (check_liar_ego(who, s)) return 1;
  if (ego_arch && ph_arch_fits(s.spec, ego_arch)) return 1;   // before the first launch, as every member's arch
  if (ego_arch && (uintptr_t)s.ego_params % 16 != 0) return fail_who(who, ": params must be 16-byte aligned");
  if (pool_members(ctx, who, s.spec, s.members, member_archs, member_adaps, s.n_members, s.n) || check_liar_one_hot(who, ctx, s.spec, s.n) ||
      check_pool_clones(who, ctx, s.spec))
    return 1;
  if (!deal_only && (ego_pos < 0 || ego_pos >= s.ego_rb->T)) return fail_who(who, ": ego_pos out of range (buffer full?)");
  const ph::PoolBook book{s.n, s.n_members, s.resample, s.pool_seed, ctx->pool_dev, s.partnerid, s.alt_acted, s.can, s.es_alt};
  return liar_step_run(
      ctx, g, book, liar_train_end(s, ego_pos, deal_only), counter, deal_only, {counter, 2 * counter, 2 * counter + 1},
      LiarSeats{nullptr, s.partnerid, nullptr},   // the log names the member at seat 1
      [&](unsigned long long c) {
        return seat_forward(ctx, s.spec, ego_arch, s.ego_params, s.obs_ego, s.n, s.ego_seed, c, s.ego_actions, s.ego_values,
                            s.ego_log_probs, s.ego_rb, ego_pos, s.ego_episode_start);
      },
      // every table's member -- behind a deal the freshly sampled one -- moves: one grouped launch
      [&](const float* obs, const unsigned char* active, unsigned long long c) {
        return pool_forward(ctx, who, s.spec, s.n_members, obs, s.partnerid, active, s.can, c, s.alt_actions, s.es_alt, s.n);
      },
      [&](int) { return pool_adap_redraw(ctx, s.members, member_adaps, s.n_members, counter, g); });
}

// ---- cross-play evaluation of Liar's Dice (ph_xplay.h; tester.py:41-63 over n tables) ----
int ph_liar_xplay_step(ph_ctx* ctx, const ph_liar_xplay* xp, const ph_arch* const* member_archs,
                       const ph_pool_adap* const* member_adaps, unsigned long long counter, int deal_only) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_liar_xplay_step";
  if (!ctx || !xp) return fail_who(who, ": null argument");
  const ph_liar_xplay& s = *xp;
  const ph::LiarGame g = ph::liar_game_of(s);
  if (check_liar_game(who, g)) return 1;
  if (!s.spec || !s.pairs || !s.ego_id || !s.alt_id || !s.games || !s.playing || !s.tables_left || !s.ep_return || !s.ep_length ||
      !s.returns || !s.lengths)
    return fail_who(who, ": incomplete description");
  if (s.episodes_per_table < 1) return fail_who(who, ": episodes_per_table must be at least 1");
  if (s.n_pairs < 1 || s.n_pairs > s.n) return fail_who(who, ": 1..n pairs (every pair needs a table)");
  if (!s.members) return fail_who(who, ": null member array");
  if (s.n_members < 1 || s.n_members > PH_MAX_POOL) return fail_who(who, ": the population holds 1..PH_MAX_POOL members");
  for (int k = 0; k < s.n_members; ++k)
    if (s.members[k].kind == PH_POOL_LEARNER)
      return fail("ph_liar_xplay_step: member " + std::to_string(k) + " is a PH_POOL_LEARNER: an evaluation seats frozen, cloned and scripted members only");
  for (int p = 0; p < 2 * s.n_pairs; ++p)
    if (s.pairs[p] < 0 || s.pairs[p] >= s.n_members)
      return fail("ph_liar_xplay_step: pair " + std::to_string(p / 2) + " names a member out of range");
  if (pool_members(ctx, who, s.spec, s.members, member_archs, member_adaps, s.n_members, s.n) || check_liar_one_hot(who, ctx, s.spec, s.n) ||
      check_pool_clones(who, ctx, s.spec))
    return 1;
  const ph::EvalEnd end{s.episodes_per_table, s.games, s.playing, s.tables_left, s.ep_return, s.ep_length, s.returns, s.lengths};
  // a seat's forward is one grouped launch over the member table, indexed by ego_id / alt_id; nothing is recorded
  auto seat = [&](const float* obs, const int* id, const unsigned char* active, unsigned long long c, int* actions) {
    return pool_forward(ctx, who, s.spec, s.n_members, obs, id, active, active, c, actions, nullptr, s.n);
  };
  return liar_step_run(
      ctx, g, ph::NoBook{}, end, counter, deal_only, {3 * counter, 3 * counter + 1, 3 * counter + 2}, LiarSeats{s.ego_id, s.alt_id, s.playing},
      [&](unsigned long long c) { return seat(s.obs_ego, s.ego_id, s.playing, c, s.ego_actions); },
      [&](const float* obs, const unsigned char* active, unsigned long long c) { return seat(obs, s.alt_id, active, c, s.alt_actions); },
      [&](int) { return pool_adap_redraw(ctx, s.members, member_adaps, s.n_members, counter, g); });
}
}  // namespace
}  // extern "C++"

int ph_liar_pool_step_arch(ph_ctx* ctx, const ph_liar_pool* pool, const ph_arch* ego_arch, const ph_arch* const* member_archs, int ego_pos,
                           unsigned long long counter, int deal_only) {
  return ph_liar_pool_step(ctx, pool, ego_arch, member_archs, nullptr, ego_pos, counter, deal_only);
}
int ph_liar_pool_step_adap(ph_ctx* ctx, const ph_liar_pool* pool, const ph_arch* ego_arch, const ph_arch* const* member_archs,
                           const ph_pool_adap* const* member_adaps, int ego_pos, unsigned long long counter, int deal_only) {
  return ph_liar_pool_step(ctx, pool, ego_arch, member_archs, member_adaps, ego_pos, counter, deal_only);
}
int ph_liar_pool_step(ph_ctx* ctx, const ph_liar_pool* pool, int ego_pos, unsigned long long counter, int deal_only) {
  return ph_liar_pool_step_arch(ctx, pool, nullptr, nullptr, ego_pos, counter, deal_only);
}

int ph_liar_xplay_step_arch(ph_ctx* ctx, const ph_liar_xplay* xp, const ph_arch* const* member_archs, unsigned long long counter,
                            int deal_only) {
  return ph_liar_xplay_step(ctx, xp, member_archs, nullptr, counter, deal_only);
}
int ph_liar_xplay_step_adap(ph_ctx* ctx, const ph_liar_xplay* xp, const ph_arch* const* member_archs,
                            const ph_pool_adap* const* member_adaps, unsigned long long counter, int deal_only) {
  return ph_liar_xplay_step(ctx, xp, member_archs, member_adaps, counter, deal_only);
}
int ph_liar_xplay_step(ph_ctx* ctx, const ph_liar_xplay* xp, unsigned long long counter, int deal_only) {
  return ph_liar_xplay_step_arch(ctx, xp, nullptr, counter, deal_only);
}

int ph_xplay_stats(ph_ctx* ctx, const float* returns, const int* lengths, const int* games, int n, int episodes_per_table, int n_pairs,
                   double* stats) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!returns || !lengths || !games || !stats) return fail("ph_xplay_stats: null argument");
  if (n <= 0 || episodes_per_table < 1) return fail("ph_xplay_stats: n and episodes_per_table must be positive");
  if (n_pairs < 1 || n_pairs > n) return fail("ph_xplay_stats: 1..n pairs (every pair needs a table)");
  if ((uintptr_t)stats % 16) return fail("ph_xplay_stats: stats must be 16-byte aligned");
  PH_HIP(ph::launch_xplay_stats(returns, lengths, games, n, episodes_per_table, n_pairs, stats, ctx->stream));
  return 0;
}

// ---- episode returns and lengths of a filled rollout buffer, per pool member (ph_episode.h) ----
int ph_episode_stats(ph_ctx* ctx, const ph_episode_scan* scan) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_episode_stats";
  static_assert(ph::EPISODE_NSTAT == PH_EPISODE_NSTAT, "episode statistics per member");
  if (!ctx) return fail("null ctx");
  if (!scan) return fail_who(who, ": null description");
  const ph_episode_scan& s = *scan;
  if (check_rb(s.rb)) return 1;
  if (s.T < 1 || s.T > s.rb->T) return fail_who(who, ": T must be 1..rb->T rows");
  if (s.n_members < 1 || s.n_members > PH_MAX_POOL) return fail_who(who, ": n_members must be 1..PH_MAX_POOL");
  if (s.n_members > 1 && !s.member) return fail_who(who, ": n_members > 1 needs the member array");
  if (s.resample != PH_POOL_ROBIN && s.resample != PH_POOL_RANDOM) return fail_who(who, ": unknown resample rule");
  if (!s.last_dones || !s.carry_return || !s.carry_length || !s.carry_valid || !s.stats) return fail_who(who, ": incomplete description");
  if ((uintptr_t)s.stats % 8 || ((uintptr_t)s.carry_return | (uintptr_t)s.carry_length | (uintptr_t)s.member) % 4)
    return fail_who(who, ": stats must be 8-byte aligned, carry_return / carry_length / member 4-byte aligned");
  const int E = s.rb->E;
  if (ensure(ctx, ctx->ep_partial, ctx->ep_partial_cap, (size_t)ph::episode_workgroups(E) * PH_MAX_POOL * PH_EPISODE_NSTAT)) return 1;
  if (!ctx->ep_ticket) {
    if (ctx->capturing) return fail_who(who, ": first use inside graph capture: call it once outside capture first");
    PH_HIP(hipMalloc((void**)&ctx->ep_ticket, sizeof(unsigned int)));
    PH_HIP(hipMemsetAsync(ctx->ep_ticket, 0, sizeof(unsigned int), ctx->stream));   // ordered in front of the first scan's launch
  }
  ph::EpisodeScan a;
  a.rewards = s.rb->rewards;
  a.starts = s.rb->episode_starts;
  a.last_dones = s.last_dones;
  a.T = s.T;
  a.E = E;
  a.carry_return = s.carry_return;
  a.carry_length = s.carry_length;
  a.carry_valid = s.carry_valid;
  a.K = s.n_members;
  a.member = s.n_members > 1 ? s.member : nullptr;
  a.resample = s.resample;
  a.pool_seed = s.pool_seed;
  a.counter0 = s.counter0;
  a.epoch = ctx->rng_epoch;
  a.stats = s.stats;
  a.partial = ctx->ep_partial;
  a.ticket = ctx->ep_ticket;
  PH_HIP(ph::launch_episode_scan(a, ctx->stream));
  return 0;
}

// ---- the device-resident move log of the Liar's Dice steps (ph_record.h) ----
namespace {
int check_liar_record(const char* who, const ph_liar_record* rec) {
  if (!rec) return fail_who(who, ": null recorder");
  if (rec->n < 1) return fail_who(who, ": n must be positive");
  if (rec->cap < 1) return fail_who(who, ": cap must be at least 1");
  if (!rec->rows || !rec->count || !rec->count_alt || !rec->dropped || !rec->pending) return fail_who(who, ": incomplete recorder");
  if ((uintptr_t)rec->rows % 16) return fail_who(who, ": rows must be 16-byte aligned");
  if (((uintptr_t)rec->member | (uintptr_t)rec->count | (uintptr_t)rec->count_alt | (uintptr_t)rec->dropped | (uintptr_t)rec->pending) % 4)
    return fail_who(who, ": member / count / count_alt / dropped / pending must be 4-byte aligned");
  return 0;
}
ph::RecordLog record_log_of(const ph_liar_record& r) {
  return ph::RecordLog{r.n, r.cap, r.rows, r.member, r.count, r.count_alt, r.dropped, r.pending};
}
}  // namespace

int ph_liar_record_attach(ph_ctx* ctx, const ph_liar_record* rec) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_liar_record_attach";
  if (!ctx) return fail("null ctx");
  // a captured step holds the launches of the recorder it was captured with: attaching or detaching inside capture would leave
  // the graph and the context in disagreement
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (ctx->stream) PH_HIP(hipStreamIsCapturing(ctx->stream, &cap));
  if (ctx->capturing || cap != hipStreamCaptureStatusNone)
    return fail_who(who, ": refused inside graph capture (attach the recorder before capture begins)");
  if (!rec) {
    ctx->recording = false;
    ctx->rec = ph::RecordLog{};
    return 0;
  }
  if (check_liar_record(who, rec)) return 1;
  ctx->rec = record_log_of(*rec);
  ctx->recording = true;
  return 0;
}

int ph_liar_record_export(ph_ctx* ctx, const ph_liar_record* rec, int seat, long long* offsets, float* rows_out, int* member_out,
                          long long out_cap) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_liar_record_export";
  if (!ctx) return fail("null ctx");
  if (check_liar_record(who, rec)) return 1;
  if (seat < -1 || seat > 1) return fail_who(who, ": seat must be -1 (every row), 0 or 1");
  if (!offsets) return fail_who(who, ": null offsets");
  if ((uintptr_t)offsets % 8 || (uintptr_t)rows_out % 4 || (uintptr_t)member_out % 4) return fail_who(who, ": misaligned output");
  if (out_cap < 0 || (member_out && !rows_out)) return fail_who(who, ": bad output arguments");
  PH_HIP(ph::launch_record_export(record_log_of(*rec), seat, offsets, rows_out, member_out, out_cap, ctx->stream));
  return 0;
}

// ---- the block worlds (ph_block.h / ph_block.hip) ----
int ph_block_reset(ph_ctx* ctx, int variant, int* state, const unsigned char* reset_mask, unsigned long long seed,
                   unsigned long long counter, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!state) return fail("ph_block_reset: null argument");
  if (variant != 0 && variant != 1) return fail("ph_block_reset: variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)");
  if (n <= 0) return fail("ph_block_reset: n must be positive");
  if ((uintptr_t)state % 16) return fail("ph_block_reset: state must be 16-byte aligned");
  PH_HIP(ph::launch_block_reset(variant, state, reset_mask, seed, counter, ctx->rng_epoch, n, ctx->stream));
  return 0;
}

int ph_block_step(ph_ctx* ctx, int variant, int* state, const int* actions, int is_ego, const unsigned char* active,
                  float* obs_next, float* rewards, unsigned char* done, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!state || !actions || !obs_next || !rewards || !done) return fail("ph_block_step: null argument");
  if (variant != 0 && variant != 1) return fail("ph_block_step: variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)");
  if (n <= 0) return fail("ph_block_step: n must be positive");
  if ((uintptr_t)state % 16) return fail("ph_block_step: state must be 16-byte aligned");
  PH_HIP(ph::launch_block_step(variant, state, actions, is_ego != 0, active, obs_next, rewards, done, n, ctx->stream));
  return 0;
}

int ph_block_obs(ph_ctx* ctx, int variant, const int* state, int is_ego, const unsigned char* active, float* obs_out, int n) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!state || !obs_out) return fail("ph_block_obs: null argument");
  if (variant != 0 && variant != 1) return fail("ph_block_obs: variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)");
  if (n <= 0) return fail("ph_block_obs: n must be positive");
  if ((uintptr_t)state % 16) return fail("ph_block_obs: state must be 16-byte aligned");
  PH_HIP(ph::launch_block_obs(variant, state, is_ego != 0, active, obs_out, n, ctx->stream));
  return 0;
}

namespace {
// the launch sequence of one vectorised block-world step, written once (seat_forward: 64-wide kernels or towers per seat)
int block_selfplay_step_run(const char* who, ph_ctx* ctx, const ph_block_selfplay* sp, const ph_arch* ego_arch, const ph_arch* alt_arch,
                            int ego_pos, unsigned long long counter) {
  const std::string w(who);
  if (!ctx || !sp) return fail(w + ": null argument");
  const ph_block_selfplay& s = *sp;
  if (s.variant != 0 && s.variant != 1) return fail(w + ": variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)");
  if (s.n <= 0) return fail(w + ": n must be positive");
  if (!s.ego_spec || !s.alt_spec || !s.ego_rb || !s.alt_rb || !s.state || !s.ego_actions || !s.alt_actions || !s.ego_episode_start ||
      !s.alt_pos || !s.alt_boundary || !s.alt_term || !s.alt_open || !s.alt_acted || !s.obs_ego || !s.obs_alt || !s.episodes ||
      !s.es_alt || !s.running || !s.can || !s.done)
    return fail(w + ": incomplete description");
  if (check_rb(s.ego_rb) || check_rb(s.alt_rb)) return 1;
  if (s.ego_rb->E != s.n || s.alt_rb->E != s.n) return fail(w + ": buffers must have E = n");
  if ((uintptr_t)s.state % 16) return fail(w + ": state must be 16-byte aligned");
  if (ego_pos < 0 || ego_pos >= s.ego_rb->T) return fail(w + ": ego_pos out of range (buffer full?)");
  // the specs must be the variant's: the book-keeping kernels write rows of these lengths
  ph_layout le, la;
  if (ph_layout_of(s.ego_spec, &le) || ph_layout_of(s.alt_spec, &la)) return 1;
  if (le.D != ph::bw_ego_obs_len(s.variant) || le.A != 1 || le.L != ph::bw_tokens(s.variant) ||
      la.D != ph::bw_alt_obs_len(s.variant) || la.A != ph::bw_alt_act_len(s.variant))
    return fail(w + ": the specs are not the variant's planner / constructor spaces");
  // the planner moves in every table
  if (seat_forward(ctx, s.ego_spec, ego_arch, s.ego_params, s.obs_ego, s.n, s.ego_seed, counter, s.ego_actions, s.ego_values,
                   s.ego_log_probs, s.ego_rb, ego_pos, s.ego_episode_start))
    return 1;
  PH_HIP(ph::launch_block_sp_after_ego(s, s.ego_rb->rewards + (size_t)ego_pos * s.n, counter, ctx->rng_epoch, ctx->stream));
  // the constructor replies where the game goes on
  if (seat_forward_ragged(ctx, s.alt_spec, alt_arch, s.alt_params, s.obs_alt, s.alt_seed, counter, s.alt_actions, s.alt_values,
                          s.alt_log_probs, s.alt_rb, s.alt_pos, s.can, s.es_alt))
    return 1;
  PH_HIP(ph::launch_block_sp_after_alt(s, ctx->stream));
  return 0;
}
}  // namespace

int ph_block_selfplay_step(ph_ctx* ctx, const ph_block_selfplay* sp, int ego_pos, unsigned long long counter) {
  DevGuard dev_guard(ctx);
  return block_selfplay_step_run("ph_block_selfplay_step", ctx, sp, nullptr, nullptr, ego_pos, counter);
}

int ph_block_selfplay_step_arch(ph_ctx* ctx, const ph_block_selfplay* sp, const ph_arch* ego_arch, const ph_arch* alt_arch, int ego_pos,
                                unsigned long long counter) {
  DevGuard dev_guard(ctx);
  return block_selfplay_step_run("ph_block_selfplay_step_arch", ctx, sp, ego_arch, alt_arch, ego_pos, counter);
}

int ph_block_replay_host(int variant, int n, int rounds, int* state, const int* tokens, const int* alt_actions, float* alt_obs_out,
                         float* rewards_out, unsigned char* done_out, float* ego_obs_out, int do_reset, unsigned long long seed,
                         unsigned long long counter, int max_draws) {
  if (variant != 0 && variant != 1) return fail("ph_block_replay_host: variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)");
  if (!state || n <= 0 || rounds < 0) return fail("ph_block_replay_host: bad arguments");
  if (rounds > 0 && (!tokens || !alt_actions)) return fail("ph_block_replay_host: moves missing");
  const int Da = ph::bw_alt_obs_len(variant), De = ph::bw_ego_obs_len(variant), A = ph::bw_alt_act_len(variant);
  for (int e = 0; e < n; ++e) {
    ph::BwTable t;
    int* w = state + (size_t)e * ph::BW_WORDS;
    if (do_reset) ph::bw_reset(t, variant, seed, counter, (uint32_t)e, max_draws < 0 ? ph::BW_MAX_DRAWS : max_draws);
    else ph::bw_unpack(t, variant, w);
    for (int r = 0; r < rounds; ++r) {
      const size_t i = (size_t)r * n + e;
      const ph::BwOutcome o = ph::bw_ego_step(t, variant, tokens[i]);
      if (alt_obs_out) ph::bw_write_alt_obs(t, variant, alt_obs_out + i * Da);
      if (rewards_out) rewards_out[2 * i] = rewards_out[2 * i + 1] = o.reward;
      if (done_out) done_out[i] = o.done ? 1 : 0;
      int a[3] = {alt_actions[i * A], alt_actions[i * A + 1], variant ? alt_actions[i * A + 2] : 0};
      ph::bw_alt_step(t, variant, a);
      if (ego_obs_out) ph::bw_write_ego_obs(t, variant, ego_obs_out + i * De);
    }
    ph::bw_pack(t, variant, w);
  }
  return 0;
}

// ---- cross-play evaluation of the block worlds: scripted constructors, the grouped forward, the step ----
namespace {
int check_block_rule(const char* who, int variant, int rule) {
  if (variant != 0 && variant != 1) return fail_who(who, ": variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)");
  if (rule != PH_BLOCK_RULE_DEFAULT && rule != PH_BLOCK_RULE_EASY) return fail_who(who, ": unknown rule (PH_BLOCK_RULE_DEFAULT / PH_BLOCK_RULE_EASY)");
  if (rule == PH_BLOCK_RULE_EASY && variant != 0) return fail_who(who, ": PH_BLOCK_RULE_EASY (SBWEasyPartner) exists for BlockEnv-v0 only");
  return 0;
}
// the variant whose constructor spaces the layout describes, -1 when it describes neither's
int block_constructor_variant(const ph_layout& l) {
  for (int v = 0; v < 2; ++v)
    if (l.D == ph::bw_alt_obs_len(v) && l.A == ph::bw_alt_act_len(v) && l.L == (v ? 11 : 8) && l.F == (v ? 30 + 3 * ph::BW_CELLS : 16 + 19 * ph::BW_BLOCKS))
      return v;
  return -1;
}
// validate the members of one seat and bring that seat's device-side table up to date (pool_members' manner: uploaded only when it
// changed, never inside graph capture).  ctor_variant: the variant whose constructor the spec is, -1: scripted members are refused.
// learner_n: 0 -- an evaluation: learners are refused; n > 0 -- the block worlds' partner pool: a learner brings a buffer of E = n
// and its per-table book (pool_members' checks).
int group_members(ph_ctx* ctx, const char* who, int table, int ctor_variant, const ph_pool_member* members, int K, int learner_n = 0) {
  const std::string w(who);
  if (!members) return fail(w + ": null member array");
  if (K < 1 || K > PH_MAX_POOL) return fail(w + ": a seat holds 1..PH_MAX_POOL members");
  ph::PoolMemberDev tab[PH_MAX_POOL];
  const size_t used = sizeof(ph::PoolMemberDev) * (size_t)K;
  std::memset(tab, 0, used);
  bool scripted = false, frozen = false, learner = false;
  for (int k = 0; k < K; ++k) {
    const ph_pool_member& m = members[k];
    ph::PoolMemberDev& d = tab[k];
    const std::string wk = w + ": member " + std::to_string(k);
    if (m.kind == PH_POOL_LEARNER && !learner_n) return fail(wk + " is a PH_POOL_LEARNER: an evaluation seats frozen and scripted members only");
    if (m.kind == PH_POOL_CLONE) return fail(wk + " is a PH_POOL_CLONE: a BC clone does not sit in the block worlds' grouped forward");
    if (m.kind != PH_POOL_FROZEN && m.kind != PH_POOL_SCRIPTED && m.kind != PH_POOL_LEARNER) return fail(wk + ": unknown kind");
    d.kind = d.fwd = m.kind;
    if (m.kind == PH_POOL_SCRIPTED) {
      if (ctor_variant < 0) return fail(wk + ": a scripted member needs a block-world constructor spec");
      if (check_block_rule(wk.c_str(), ctor_variant, m.seed > 1ull ? -1 : (int)m.seed)) return 1;   // (`seed` holds the rule)
      d.rb_T = (int)m.seed;
      scripted = true;
      continue;
    }
    if (!m.params) return fail(wk + ": null params");
    if ((uintptr_t)m.params % 16 != 0) return fail(wk + ": params must be 16-byte aligned");
    d.params = m.params;
    d.seed = m.seed;
    if (m.kind == PH_POOL_FROZEN) {
      frozen = true;
      continue;
    }
    if (!m.rb) return fail(wk + ": a learner needs its rollout buffer");
    if (check_rb(m.rb)) return 1;
    if (m.rb->E != learner_n) return fail(wk + ": the learner's buffer must have E = n");
    if (!m.pos || !m.boundary || !m.term || !m.open || !m.values || !m.log_probs)
      return fail(wk + ": a learner needs pos / boundary / term / open / values / log_probs");
    d.values = m.values;
    d.log_probs = m.log_probs;
    d.rb_T = m.rb->T;
    d.rb_obs = m.rb->observations;
    d.rb_act = m.rb->actions;
    d.rb_rew = m.rb->rewards;
    d.rb_es = m.rb->episode_starts;
    d.rb_val = m.rb->values;
    d.rb_logp = m.rb->log_probs;
    d.pos = m.pos;
    d.boundary = m.boundary;
    d.term = m.term;
    d.open = m.open;
    learner = true;
  }
  if (ctx->group_count[table] != K || std::memcmp(ctx->group_host[table], tab, used) != 0) {
    if (ctx->capturing) return fail(w + ": the member table changed inside graph capture: run the same call once outside capture first");
    if (!ctx->group_dev[table]) PH_HIP(hipMalloc((void**)&ctx->group_dev[table], sizeof(tab)));
    PH_HIP(hipStreamSynchronize(ctx->stream));   // launches in flight still read the table
    std::memcpy(ctx->group_host[table], tab, used);
    ctx->group_count[table] = 0;
    PH_HIP(hipMemcpyAsync(ctx->group_dev[table], ctx->group_host[table], used, hipMemcpyHostToDevice, ctx->stream));
    PH_HIP(hipStreamSynchronize(ctx->stream));
    ctx->group_count[table] = K;
    ctx->group_scripted[table] = scripted;
    ctx->group_frozen[table] = frozen;
    ctx->group_learner[table] = learner;
  }
  return 0;
}
// the spec's member table (block_constructor_variant into *ctor_variant) -- before anything is launched
int group_table_of(const ph_spec* spec, int* ctor_variant) {
  ph_layout lay;
  if (layout_of(spec, &lay)) return -1;
  *ctor_variant = block_constructor_variant(lay);
  return *ctor_variant >= 0 ? 1 : 0;
}
// bucket pass + the frozen members' tiles + the scripted members' rows over the tables with active[e] != 0.  A table that holds a
// learner (the partner pool): its learners' and frozen members' tiles in launch_group_learn's ONE launch instead, the learners' rows
// recorded where rec_mask[e] != 0 with es_in[e].
int group_forward(ph_ctx* ctx, const char* who, int table, int ctor_variant, const ph_spec* spec, int K, const float* obs,
                  const int* member_of, const unsigned char* active, unsigned long long counter, int* actions, int n,
                  const unsigned char* rec_mask = nullptr, const float* es_in = nullptr) {
  ph::PoolFwd p;
  std::memset(&p, 0, sizeof(p));
  if (fwd_args(p.a, ctx, spec, false, nullptr, obs, n, 0, counter, actions, nullptr, nullptr)) return 1;
  if (!ph::group_fwd_eligible(p.a.nd, n))
    return fail_who(who, ": the spec is not in the grouped forward's class (categorical heads of at most 32 logits, n < 16384, not the "
                         "16-row dense class of one Discrete head of <= 8 logits over one feature chunk)");
  const bool learner = ctx->group_learner[table];
  if (learner && !ph::group_learn_eligible(p.a.nd, n))
    return fail_who(who, ": the member table holds a PH_POOL_LEARNER, whose tiles exist on the 16-row one-hot forward only (one-hot "
                         "observations of at most 64 components, PH_FWD16H not 0): the spec is not in that class");
  if (learner && (!rec_mask || !es_in)) return fail_who(who, ": learners need a record mask and episode_start_in");
  p.a.rec_mask = learner ? rec_mask : nullptr;
  p.a.es_in = learner ? es_in : nullptr;
  if (ctx->group_frozen[table] || learner) {
    if (ensure(ctx, ctx->pool_order, ctx->pool_order_cap, (size_t)n)) return 1;
    const size_t ntile = (size_t)ph::pool_max_tiles(n, PH_MAX_POOL);
    if (ensure(ctx, ctx->pool_tiles, ctx->pool_tiles_cap, 3 * (ntile + 1))) return 1;
    p.members = ctx->group_dev[table];
    p.b.order = ctx->pool_order;
    p.b.tiles = ctx->pool_tiles;
    p.b.ntiles = ctx->pool_tiles + 3 * ntile;
    PH_HIP(ph::launch_pool_bucket(member_of, active, n, K, p.b, ctx->stream));
    PH_HIP(learner ? ph::launch_group_learn(p, K, ctx->stream) : ph::launch_group_fwd(p, K, ctx->stream));
  }
  if (ctx->group_scripted[table])
    PH_HIP(ph::launch_block_group_scripted(ctor_variant, obs, ctx->group_dev[table], member_of, active, actions, n, K, ctx->stream));
  return 0;
}
}  // namespace

int ph_block_scripted_actions(ph_ctx* ctx, int variant, int rule, const float* obs, const unsigned char* active, int* actions, int n) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_block_scripted_actions";
  if (!ctx) return fail("null ctx");
  if (!obs || !actions) return fail_who(who, ": null argument");
  if (n <= 0) return fail_who(who, ": n must be positive");
  if (check_block_rule(who, variant, rule)) return 1;
  PH_HIP(ph::launch_block_scripted_actions(variant, rule, obs, active, actions, n, ctx->stream));
  return 0;
}

int ph_block_scripted_actions_host(int variant, int rule, const float* obs, int* actions, int n) {
  const char* who = "ph_block_scripted_actions_host";
  if (!obs || !actions || n <= 0) return fail_who(who, ": bad arguments");
  if (check_block_rule(who, variant, rule)) return 1;
  const int D = ph::bw_alt_obs_len(variant), A = ph::bw_alt_act_len(variant);
  for (int e = 0; e < n; ++e) {
    int a[3];
    ph::bw_scripted_move(variant, rule, obs + (size_t)e * D, a);
    for (int j = 0; j < A; ++j) actions[(size_t)e * A + j] = a[j];
  }
  return 0;
}

int ph_block_group_forward(ph_ctx* ctx, const ph_spec* spec, const ph_pool_member* members, int n_members, const float* obs,
                           const int* member_of, const unsigned char* active, unsigned long long counter, int* actions, int n) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_block_group_forward";
  if (!ctx) return fail("null ctx");
  if (!spec || !obs || !member_of || !active || !actions) return fail_who(who, ": null argument");
  if (n <= 0) return fail_who(who, ": n must be positive");
  int ctor_variant = -1;
  const int table = group_table_of(spec, &ctor_variant);
  if (table < 0) return 1;
  if (group_members(ctx, who, table, ctor_variant, members, n_members)) return 1;
  return group_forward(ctx, who, table, ctor_variant, spec, n_members, obs, member_of, active, counter, actions, n);
}

int ph_block_xplay_step(ph_ctx* ctx, const ph_block_xplay* xp, unsigned long long counter, int first) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_block_xplay_step";
  if (!ctx || !xp) return fail_who(who, ": null argument");
  const ph_block_xplay& s = *xp;
  if (s.variant != 0 && s.variant != 1) return fail_who(who, ": variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)");
  if (s.n <= 0) return fail_who(who, ": n must be positive");
  if (!s.ego_spec || !s.alt_spec || !s.state || !s.pairs || !s.ego_id || !s.alt_id || !s.ego_actions || !s.alt_actions || !s.obs_ego ||
      !s.obs_alt || !s.games || !s.playing || !s.tables_left || !s.ep_return || !s.ep_length || !s.returns || !s.lengths || !s.running)
    return fail_who(who, ": incomplete description");
  if ((uintptr_t)s.state % 16) return fail_who(who, ": state must be 16-byte aligned");
  if (s.episodes_per_table < 1) return fail_who(who, ": episodes_per_table must be at least 1");
  if (s.n_pairs < 1 || s.n_pairs > s.n) return fail_who(who, ": 1..n pairs (every pair needs a table)");
  ph_layout le, la;
  if (ph_layout_of(s.ego_spec, &le) || ph_layout_of(s.alt_spec, &la)) return 1;
  if (le.D != ph::bw_ego_obs_len(s.variant) || le.A != 1 || le.L != ph::bw_tokens(s.variant) || block_constructor_variant(la) != s.variant)
    return fail_who(who, ": the specs are not the variant's planner / constructor spaces");
  if (s.n_planners < 1 || s.n_planners > PH_MAX_POOL || s.n_constructors < 1 || s.n_constructors > PH_MAX_POOL)
    return fail_who(who, ": a seat holds 1..PH_MAX_POOL members");
  for (int p = 0; p < s.n_pairs; ++p)
    if (s.pairs[2 * p] < 0 || s.pairs[2 * p] >= s.n_planners || s.pairs[2 * p + 1] < 0 || s.pairs[2 * p + 1] >= s.n_constructors)
      return fail("ph_block_xplay_step: pair " + std::to_string(p) + " names a member out of range");
  if (group_members(ctx, "ph_block_xplay_step: planners", 0, -1, s.planners, s.n_planners) ||
      group_members(ctx, "ph_block_xplay_step: constructors", 1, s.variant, s.constructors, s.n_constructors))
    return 1;
  if (first) {
    PH_HIP(ph::launch_block_reset(s.variant, s.state, nullptr, s.world_seed, 0ull, ctx->rng_epoch, s.n, ctx->stream));
    PH_HIP(ph::launch_block_obs(s.variant, s.state, 1, nullptr, s.obs_ego, s.n, ctx->stream));
    return 0;
  }
  if (group_forward(ctx, who, 0, -1, s.ego_spec, s.n_planners, s.obs_ego, s.ego_id, s.playing, 2 * counter, s.ego_actions, s.n)) return 1;
  PH_HIP(ph::launch_block_xp_after_ego(s, counter, ctx->rng_epoch, ctx->stream));
  if (group_forward(ctx, who, 1, s.variant, s.alt_spec, s.n_constructors, s.obs_alt, s.alt_id, s.running, 2 * counter + 1, s.alt_actions,
                    s.n))
    return 1;
  PH_HIP(ph::launch_block_xp_after_alt(s, ctx->stream));
  return 0;
}

// ---- the block worlds against a pool of constructors: the grouped forward with learners, the step ----
int ph_block_pool_forward(ph_ctx* ctx, const ph_spec* spec, const ph_pool_member* members, int n_members, const float* obs,
                          const int* member_of, const unsigned char* active, unsigned long long counter, int* actions,
                          const float* episode_start_in, int n) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_block_pool_forward";
  if (!ctx) return fail("null ctx");
  if (!spec || !obs || !member_of || !active || !actions) return fail_who(who, ": null argument");
  if (n <= 0) return fail_who(who, ": n must be positive");
  int ctor_variant = -1;
  const int table = group_table_of(spec, &ctor_variant);
  if (table < 0) return 1;
  if (members && n_members >= 1 && n_members <= PH_MAX_POOL)
    for (int k = 0; k < n_members; ++k)
      if (members[k].kind == PH_POOL_LEARNER && !episode_start_in) return fail_who(who, ": learners need episode_start_in");
  if (group_members(ctx, who, table, ctor_variant, members, n_members, n)) return 1;
  return group_forward(ctx, who, table, ctor_variant, spec, n_members, obs, member_of, active, counter, actions, n, active,
                       episode_start_in);
}

int ph_block_pool_step(ph_ctx* ctx, const ph_block_pool* pool, int ego_pos, unsigned long long counter, int first) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_block_pool_step";
  if (!ctx || !pool) return fail_who(who, ": null argument");
  const ph_block_pool& s = *pool;
  if (s.variant != 0 && s.variant != 1) return fail_who(who, ": variant must be 0 (BlockEnv-v0) or 1 (BlockEnv-v1)");
  if (s.n <= 0) return fail_who(who, ": n must be positive");
  if (!s.ego_spec || !s.alt_spec || !s.state || !s.ego_params || !s.ego_rb || !s.ego_actions || !s.ego_episode_start || !s.partnerid ||
      !s.alt_actions || !s.alt_acted || !s.obs_ego || !s.obs_alt || !s.episodes || !s.es_alt || !s.running || !s.can || !s.done)
    return fail_who(who, ": incomplete description");
  if (s.resample != PH_POOL_ROBIN && s.resample != PH_POOL_RANDOM) return fail_who(who, ": unknown resample rule");
  if (check_rb(s.ego_rb)) return 1;
  if (s.ego_rb->E != s.n) return fail_who(who, ": buffers must have E = n");
  if ((uintptr_t)s.state % 16) return fail_who(who, ": state must be 16-byte aligned");
  if ((uintptr_t)s.ego_params % 16) return fail_who(who, ": params must be 16-byte aligned");
  if (!first && (ego_pos < 0 || ego_pos >= s.ego_rb->T)) return fail_who(who, ": ego_pos out of range (buffer full?)");
  // the specs must be the variant's: the book-keeping kernels write rows of these lengths
  ph_layout le, la;
  if (ph_layout_of(s.ego_spec, &le) || ph_layout_of(s.alt_spec, &la)) return 1;
  if (le.D != ph::bw_ego_obs_len(s.variant) || le.A != 1 || le.L != ph::bw_tokens(s.variant) || block_constructor_variant(la) != s.variant)
    return fail_who(who, ": the specs are not the variant's planner / constructor spaces");
  if (group_members(ctx, "ph_block_pool_step", 1, s.variant, s.members, s.n_members, s.n)) return 1;
  {   // what the grouped forward would refuse, in front of the first launch
    ph::NetDims nd;
    if (resolve(ctx, s.alt_spec, &nd)) return 1;
    if (!ph::group_fwd_eligible(nd, s.n) || (ctx->group_learner[1] && !ph::group_learn_eligible(nd, s.n)))
      return fail_who(who, ": the constructor spec is not in the grouped forward's class -- a PH_POOL_LEARNER's tiles exist on the 16-row "
                           "one-hot forward only (PH_FWD16H not 0)");
  }
  const ph::PoolBook book{s.n, s.n_members, s.resample, s.pool_seed, ctx->group_dev[1], s.partnerid, s.alt_acted, s.can, s.es_alt};
  if (first) {
    PH_HIP(ph::launch_block_pool_after_ego(s, book, nullptr, 0ull, ctx->rng_epoch, 1, ctx->stream));
    return 0;
  }
  // the planner moves in every table
  if (seat_forward(ctx, s.ego_spec, nullptr, s.ego_params, s.obs_ego, s.n, s.ego_seed, counter, s.ego_actions, s.ego_values,
                   s.ego_log_probs, s.ego_rb, ego_pos, s.ego_episode_start))
    return 1;
  PH_HIP(ph::launch_block_pool_after_ego(s, book, s.ego_rb->rewards + (size_t)ego_pos * s.n, counter, ctx->rng_epoch, 0, ctx->stream));
  // every running table's member replies: one bucket pass, one grouped launch, the scripted rows
  if (group_forward(ctx, who, 1, s.variant, s.alt_spec, s.n_members, s.obs_alt, s.partnerid, s.running, counter, s.alt_actions, s.n, s.can,
                    s.es_alt))
    return 1;
  PH_HIP(ph::launch_block_pool_after_alt(s, book, ctx->stream));
  return 0;
}

int ph_liar_selfplay_rollout(ph_ctx* ctx, const ph_liar_selfplay* sp, int ego_pos, int n_steps, unsigned long long counter) {
  DevGuard dev_guard(ctx);
  const char* who = "ph_liar_selfplay_rollout";
  if (check_liar_selfplay(who, ctx, sp)) return 1;
  if (ctx->recording)
    return fail("ph_liar_selfplay_rollout: a recorder is attached (ph_liar_record_attach) and the one-launch rollout does not record: "
                "detach it, or step with ph_liar_selfplay_step");
  const ph_liar_selfplay& s = *sp;
  if (n_steps <= 0 || ego_pos < 0 || ego_pos > s.ego_rb->T - n_steps)
    return fail("ph_liar_selfplay_rollout: ego_pos + n_steps exceeds the ego's buffer");
  if (((uintptr_t)s.ego_params | (uintptr_t)s.alt_params) % 16) return fail("ph_liar_selfplay_rollout: params must be 16-byte aligned");
  // the argument records of ph_liar_selfplay_step's three forwards, from the helpers its forwards build them with (forward_run's
  // row, forward_ragged_run's bases); the Philox counters are the kernel's
  ph::FwdArgs ego, reply, opening;
  if (fwd_args(ego, ctx, s.spec, false, s.ego_params, s.obs_ego, s.n, s.ego_seed, 0, s.ego_actions, s.ego_values, s.ego_log_probs))
    return 1;
  if (!ph::liar_rollout_eligible(ego.nd, s.n))
    return fail("ph_liar_selfplay_rollout: the spec does not fit the 16-row one-hot forward (use ph_liar_selfplay_step)");
  if (fwd_bind_row(who, ego, s.ego_rb, ego_pos, s.ego_episode_start, nullptr)) return 1;
  ego.prof = ctx->prof;   // debug stamps (scripts/liar_rollout_profile.py)
  if (fwd_args(reply, ctx, s.spec, false, s.alt_params, s.obs_next, s.n, s.alt_seed, 0, s.alt_actions, s.alt_values, s.alt_log_probs))
    return 1;
  fwd_bind_bases(reply, s.alt_rb, s.es_alt, s.alt_pos, s.can);
  opening = reply;
  opening.obs = s.obs_alt;
  PH_HIP(ph::launch_liar_rollout(s, ego, reply, opening, n_steps, counter, ctx->rng_epoch, ego.rb_rew, ctx->stream));
  return 0;
}

int ph_framestack_push(ph_ctx* ctx, float* stack, const float* obs, const unsigned char* reset_mask,
                       const float* default_obs, int n, int D, int numframes) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!stack || !obs) return fail("ph_framestack_push: null argument");
  if (n <= 0 || D <= 0 || numframes <= 0) return fail("ph_framestack_push: bad sizes");
  PH_HIP(ph::launch_framestack_push(stack, obs, reset_mask, default_obs, n, D, numframes, ctx->stream));
  return 0;
}

// ---- K3 + K5 + K6 ----
namespace {

struct MbPlan {
  int nb, ntiles, nwg;
};

// `arch`: the towers of a run-time shape (ph_arch.hip) plan their own tile height and workgroup count
MbPlan plan_minibatch(const ph_ctx* ctx, const ph::NetDims& nd, int nb, const ph::ArchDims* arch = nullptr) {
  MbPlan p;
  p.nb = nb;
  if (arch) ph::arch_grad_plan(nd, *arch, nb, ctx->num_cu, &p.ntiles, &p.nwg);
  else ph::grad_plan(nd, nb, ctx->num_cu, &p.ntiles, &p.nwg);
  return p;
}

// ph_arch validated and resolved: offsets in the documented order (ph_arch_layout_of)
int arch_layout(const ph_spec* spec, const ph_arch* arch, ph_arch_layout* o) {
  if (!arch || !o) return fail("null arch/layout");
  ph_layout base;
  if (layout_of(spec, &base)) return 1;
  if (spec->act.kind == PH_SPACE_BOX) return fail("net_arch towers are written for the categorical heads (Discrete / MultiDiscrete actions)");
  if (arch->n_layers < 1 || arch->n_layers > PH_ARCH_MAX_LAYERS)
    return fail("ph_arch: n_layers must be between 1 and PH_ARCH_MAX_LAYERS (3)");
  for (int l = 0; l < arch->n_layers; ++l)
    if (arch->width[l] < 32 || arch->width[l] > PH_ARCH_MAX_WIDTH || arch->width[l] % 32 != 0)
      return fail("ph_arch: width " + std::to_string(arch->width[l]) + " of layer " + std::to_string(l + 1) +
                  " is not a multiple of 32 in [32, PH_ARCH_MAX_WIDTH (256)]");
  std::memset(o, 0, sizeof(*o));
  o->D = base.D; o->F = base.F; o->A = base.A; o->L = base.L;
  long long off = 0;
  for (int net = 0; net < 2; ++net) {
    int in = base.F;
    for (int l = 0; l < arch->n_layers; ++l) {
      const int w = arch->width[l];
      (net == 0 ? o->pi_W : o->vf_W)[l] = (int)off; off += (long long)in * w;
      (net == 0 ? o->pi_b : o->vf_b)[l] = (int)off; off += w;
      in = w;
    }
  }
  const int wn = arch->width[arch->n_layers - 1];
  o->act_W = (int)off; off += (long long)wn * base.L;
  o->act_b = (int)off; off += base.L;
  o->val_W = (int)off; off += wn;
  o->val_b = (int)off; off += 1;
  if (off >= (1ll << 31)) return fail("ph_arch: parameter count must fit in int32");
  o->P = (int)off;
  return 0;
}

// the smallest carve (32-row tiles: the forward launch, and the gradient launch's fall-back) must fit the CU's LDS; the one place
// that says so, for the entry points (arch_resolve) and for ph_arch_fits
int arch_lds_refusal(const ph::NetDims& nd, const ph::ArchDims& ad) {
  const size_t need = std::max(ph::arch_grad_lds_bytes(nd, ad, ph::ARCH_FWD_ROWS), ph::arch_fwd_lds_bytes(nd, ad));
  if (need > ph::ARCH_LDS_MAX)
    return fail("ph_arch: observation space too large for the tower kernels' LDS tile (" + std::to_string(need) +
                " bytes at 32 rows, " + std::to_string(ph::ARCH_LDS_MAX) + " available)");
  return 0;
}

// the dimensions the LDS carves depend on, from host descriptions alone (no context)
int arch_host_dims(const ph_spec* spec, const ph_arch* arch, ph::NetDims* nd, ph::ArchDims* ad) {
  std::memset(ad, 0, sizeof(*ad));
  if (arch_layout(spec, arch, &ad->lay)) return 1;
  ad->nl = arch->n_layers;
  for (int l = 0; l < arch->n_layers; ++l) ad->w[l] = arch->width[l];
  std::memset(nd, 0, sizeof(*nd));
  nd->obs_kind = spec->obs.kind;
  nd->D = ad->lay.D;
  nd->nchunk = (ad->lay.F + PH_HIDDEN - 1) / PH_HIDDEN;
  return 0;
}

// spec and arch resolved for the tower kernels: nd as `resolve` leaves it, minus every table of the 64-wide gradient kernels,
// with lay.P the ARCH's parameter count (slab length, reduce / Adam extent)
int arch_resolve(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, ph::NetDims* nd, ph::ArchDims* ad) {
  std::memset(ad, 0, sizeof(*ad));
  if (arch_layout(spec, arch, &ad->lay)) return 1;
  if (resolve(ctx, spec, nd, false)) return 1;
  ad->nl = arch->n_layers;
  for (int l = 0; l < arch->n_layers; ++l) ad->w[l] = arch->width[l];
  nd->slab_map = nd->slab_map_split = nd->wimage_map = nullptr;
  nd->split = nd->split_kind = 0;
  nd->lay.P = ad->lay.P;
  return arch_lds_refusal(*nd, *ad);
}

void fill_grad_args(ph::GradArgs& g, const ph::NetDims& nd, const float* params, const ph_rollout* rb,
                    const ph_ppo_hyper* hp, ph_ctx* ctx) {
  g.nd = nd;
  g.params = params;
  g.rb_obs = rb->observations;
  g.rb_act = rb->actions;
  g.rb_val = rb->values;
  g.rb_logp = rb->log_probs;
  g.rb_adv = rb->advantages;
  g.rb_ret = rb->returns;
  g.T = rb->T;
  g.E = rb->E;
  g.clip = hp->clip_range;
  g.clip_vf = hp->clip_range_vf;
  g.ent_coef = hp->ent_coef;
  g.vf_coef = hp->vf_coef;
  g.norm_adv = hp->normalize_advantage;
  g.slabs = ctx->slabs;
  g.statpart = ctx->statpart;
  g.stop_flag = ctx->stop_flag;
  g.prof = ctx->prof;
  g.wimage = ctx->wimage;
  g.ximg = ctx->ximg;
  g.ximg_zero_row = rb->T * rb->E;
  g.rec_pi = ctx->rec_pi;   // callers offset these to the minibatch
  g.rec_vf = ctx->rec_vf;
}

// the split kernel's weight fragment image of `params`, rebuilt from scratch (entries no parameter backs are zero): at the start
// of every train() / gradient call, whatever happened to the parameters in between; ppo_adam_kernel keeps it current afterwards
int rebuild_weight_image(ph_ctx* ctx, const ph::NetDims& nd, const float* params) {
  if (!nd.split) return 0;
  if ((size_t)nd.wimage_elems > ctx->wimage_cap) {
    if (ctx->capturing) return fail("first split-kernel use inside graph capture: call it once outside capture first");
    if (ensure(ctx, ctx->wimage, ctx->wimage_cap, (size_t)nd.wimage_elems)) return 1;
    ctx->wimage_zeroed_for = 0;
  }
  // Elements no parameter backs are written by nobody (weight_image_kernel / ppo_adam_kernel go through the map), so they are
  // zeroed when the image starts serving a spec, not before every call (a 4.5 us fill node in every iteration graph).  The fill
  // and every later user of the image are enqueued on the context's stream of that moment; a context whose stream is switched
  // (ph_ctx_set_stream) is synchronised by its owner at the switch, as for every other piece of workspace.
  if (ctx->wimage_zeroed_for != nd.spec_id) {
    if (ctx->capturing) return fail("the weight image changes its spec inside graph capture: run the same call once outside capture first");
    PH_HIP(hipMemsetAsync(ctx->wimage, 0, (size_t)nd.wimage_elems * sizeof(unsigned short), ctx->stream));
    ctx->wimage_zeroed_for = nd.spec_id;
  }
  PH_HIP(ph::launch_weight_image(params, ctx->wimage, nd.wimage_map, nd.lay.P, ctx->stream));
  return 0;
}

// The split kernel's gradient pack: workspace for `n_rec` row records per net and the plane image of the buffer's rows, and the
// image itself (obs_planes_kernel) -- built at the start of every train() / gradient call from the observations as they are
// then.  The row records are written by the advantage-statistics launch that follows (fill_adv_records).
int build_grad_pack(ph_ctx* ctx, const ph::NetDims& nd, const ph_rollout* rb, size_t n_rec) {
  if (nd.split != 1) return 0;   // the one-hot kernel gathers its rows itself (D integers per row: nothing to split ahead)
  const size_t rows = (size_t)rb->T * rb->E;
  const size_t need_img = (rows + 1) * ph::XIMG_ROW_U4;
  if (ensure(ctx, ctx->ximg, ctx->ximg_cap, need_img)) return 1;
  if (ensure(ctx, ctx->rowrec, ctx->rowrec_cap, 2 * rows)) return 1;
  if (n_rec > ctx->rec_cap) {
    size_t c1 = ctx->rec_cap, c2 = ctx->rec_cap;
    if (ensure(ctx, ctx->rec_pi, c1, n_rec)) return 1;
    if (ensure(ctx, ctx->rec_vf, c2, n_rec)) return 1;
    ctx->rec_cap = n_rec;
  }
  PH_HIP(ph::launch_obs_planes(rb->observations, (int)rows, nd.D, nd.F, ph::grad_fast_fold(nd) ? 1 : 0, ctx->ximg, rb->advantages,
                               rb->log_probs, rb->actions, rb->returns, rb->values, ctx->rowrec, ctx->stream));
  return 0;
}
void fill_adv_records(ph::AdvStatArgs& aa, const ph_ctx* ctx, const ph::NetDims& nd, const ph_rollout* rb) {
  aa.rec_pi_out = nd.split == 1 ? ctx->rec_pi : nullptr;
  aa.rec_vf_out = nd.split == 1 ? ctx->rec_vf : nullptr;
  aa.rowrec = (nd.split == 1 && rb->advantages && rb->log_probs && rb->actions && rb->returns && rb->values) ? ctx->rowrec : nullptr;
  aa.rb_logp = rb->log_probs;
  aa.rb_act = rb->actions;
  aa.rb_ret = rb->returns;
  aa.rb_val = rb->values;
}


// gemm_mode 2 (products as six bf16 MFMA terms over three-plane operands, float32 accuracy) applies to the gradient launches
// of specs ppo_grad_split_kernel takes; everywhere else it means 0.  The split kernel's slabs have their own order.
void select_gemm(ph::NetDims& nd, int gemm_mode) {
  nd.split = (gemm_mode == 2 && nd.slab_map_split != nullptr) ? nd.split_kind : 0;
  if (nd.split) nd.slab_map = nd.slab_map_split;
}

// floats per gradient slab: the canonical parameter layout, the register-order layout of ppo_grad_fast_kernel, or a split kernel's
int slab_len_of(const ph::NetDims& nd) { return nd.split ? nd.slab_len_split : (nd.slab_map ? 2 * ph::RS_NET : nd.lay.P); }

int ensure_train_ws(ph_ctx* ctx, int P, int slab_len, int nwg_max, int n_mb_total, size_t n_idx = 0, size_t n_phys = 0) {
  if (n_phys && ensure(ctx, ctx->perm_phys, ctx->perm_phys_cap, n_phys)) return 1;
  if (ensure(ctx, ctx->slabs, ctx->slabs_cap, (size_t)nwg_max * slab_len)) return 1;
  if (ensure(ctx, ctx->statpart, ctx->statpart_cap, (size_t)2 * nwg_max * ph::NSTATP)) return 1;
  if (ensure(ctx, ctx->grad, ctx->grad_cap, (size_t)P)) return 1;
  if (ensure(ctx, ctx->blocksq, ctx->blocksq_cap, (size_t)ph::reduce_blocks(slab_len))) return 1;
  if (ensure(ctx, ctx->advstats, ctx->advstats_cap, (size_t)n_mb_total * 2)) return 1;
  if (ensure(ctx, ctx->adam_bias, ctx->adam_bias_cap, (size_t)n_mb_total)) return 1;
  if (ensure(ctx, ctx->advpart, ctx->advpart_cap, (size_t)n_mb_total * 2 * ph::ADV_SPLIT)) return 1;
  if (n_idx && ensure(ctx, ctx->perm_idx, ctx->perm_idx_cap, n_idx)) return 1;
  const size_t n_words = (size_t)ph::reduce_blocks(slab_len) + 1;
  if (n_words > ctx->step_words_cap) {
    if (ensure(ctx, ctx->step_words, ctx->step_words_cap, n_words)) return 1;
    PH_HIP(hipMemsetAsync(ctx->step_words, 0, n_words * sizeof(unsigned long long), ctx->stream));
  }
  if (!ctx->step_gen) {
    if (ctx->capturing) return fail("workspace would grow inside graph capture: run the same call once outside capture first");
    PH_HIP(hipMalloc((void**)&ctx->step_gen, 4 * sizeof(unsigned int)));   // generation, timed-out waits, -, -
    PH_HIP(hipMemsetAsync(ctx->step_gen, 0, 4 * sizeof(unsigned int), ctx->stream));
  }
  return 0;
}

// reduce + clip + Adam of an exclusive learner's minibatch as ONE launch?
bool step_fused_wanted(const ph_ctx* ctx, int slab_len, bool alone) {
  return alone && ctx->exclusive && ctx->step_words && ctx->step_gen &&
         ph::step_fused_fits(ph::reduce_blocks(slab_len), slab_len, ctx->num_cu);
}

}  // namespace

namespace {

// one PPO.train() call resolved into launch parameters
struct TrainPlan {
  int alone = 1;          // not part of a joint call (ph_ppo_train_multi chains several learners' launches)
  ph_ctx* ctx;
  ph::NetDims nd;
  const ph_opt_state* opt;
  const ph_rollout* rb;
  const ph_ppo_hyper* hp;
  const int* perms;
  unsigned long long perm_seed;
  float* stats;
  int n_epochs, batch_size, gemm_mode, N, n_mb, P;
  uint32_t hb;
  const ph_adap_loss* adap = nullptr;   // ADAP's context term, or null = plain PPO
  bool arch = false;                    // towers of a run-time shape: arch_dims is set, the gradient launch is ph_arch.hip's
  ph::ArchDims arch_dims;
};

// ---- ADAP's context term: validation, workspace, the launch next to a minibatch's gradient launch ----
int adap_check(ph_ctx* ctx, const ph::NetDims& nd, const ph_adap_loss* ad, const char* who) {
  const std::string w(who);
  if (nd.obs_kind != PH_SPACE_BOX) return fail(w + ": the context term needs Box observations (observation ++ context)");
  if (ad->context_size <= 0 || ad->context_size >= nd.F) return fail(w + ": context_size must be in (0, observation length)");
  if (ad->num_context_samples < 2 || ad->num_context_samples > ph::ADAP_ROWS)
    return fail(w + ": num_context_samples must be in [2, 16]");
  if (ad->num_state_samples <= 0) return fail(w + ": num_state_samples must be positive");
  if (ad->sampler < PH_CTX_L2 || ad->sampler > PH_CTX_NATURAL_NUMBERS) return fail(w + ": unknown context sampler");
  if (ad->sampler == PH_CTX_NATURAL_NUMBERS && ad->context_size != 1)
    return fail(w + ": the natural_numbers sampler draws (num, 1) contexts: context_size must be 1");
  if (ph::adap_lds_bytes(nd, ad->num_context_samples, ad->context_size) > 160 * 1024)
    return fail(w + ": observation / action space too large for the context kernel's LDS tile");
  const size_t nwg = (size_t)ph::adap_workgroups(ad->num_context_samples, ad->num_state_samples);
  if (ensure(ctx, ctx->adap_extra, ctx->adap_extra_cap, nwg * ph::adap_slab_floats(nd.lay))) return 1;
  if (ensure(ctx, ctx->adap_loss, ctx->adap_loss_cap, nwg)) return 1;
  return 0;
}

// the context launch of minibatch number `mbi` (rows idx[0..nb)); fills the reduce launch's additional-term fields
int adap_launch(ph_ctx* ctx, const ph::NetDims& nd, const float* params, const ph_rollout* rb, const ph_adap_loss* ad,
                const int* idx, int nb, int mbi, ph::ReduceArgs* r) {
  const int C = ad->num_context_samples, S = ad->num_state_samples, cs = ad->context_size;
  const int n_states = S < nb ? S : nb;   // util.py:106-108
  const int nwg = ph::adap_workgroups(C, n_states);
  ph::AdapArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nd = nd;
  a.params = params;
  a.rb_obs = rb->observations;
  a.T = rb->T;
  a.E = rb->E;
  a.idx = idx;
  a.nb = nb;
  a.ctx_size = cs;
  a.n_ctx = C;
  a.n_states = n_states;
  a.sampler = ad->sampler;
  a.coef = ad->context_loss_coeff;
  a.state_idx = ad->state_idx ? ad->state_idx + (size_t)mbi * S : nullptr;
  a.contexts = ad->contexts ? ad->contexts + (size_t)mbi * C * cs : nullptr;
  a.seed = ad->seed;
  a.epoch = ctx->rng_epoch;
  a.mbi = (uint32_t)mbi;
  a.nb_hb = ph::feistel_half_bits((uint32_t)nb);
  a.extra = ctx->adap_extra;
  a.loss_part = ctx->adap_loss;
  a.used_state_idx = ad->used_state_idx ? ad->used_state_idx + (size_t)mbi * S : nullptr;
  a.used_contexts = ad->used_contexts ? ad->used_contexts + (size_t)mbi * C * cs : nullptr;
  a.stop_flag = ctx->stop_flag;
  a.prof = ctx->prof;
  PH_HIP(ph::launch_adap_context(a, nwg, ctx->stream));
  r->extra = ctx->adap_extra;
  r->n_extra = nwg;
  r->extra_len = ph::adap_slab_floats(nd.lay);
  r->extra_cut = nd.lay.vf_W1;
  r->extra_lo = nd.lay.act_W;
  r->extra_hi = nd.lay.val_W;
  r->extra_loss = ctx->adap_loss;
  r->extra_norm = 1.0f / (float)((C * (C - 1) / 2) * n_states);
  r->extra_coef = ad->context_loss_coeff;
  r->extra_loss_out = ad->context_loss ? ad->context_loss + mbi : nullptr;
  return 0;
}

// the advantage-statistics launch of a train() call: statistics of every minibatch, the minibatch order, the row records
void train_adv_args(const TrainPlan& t, bool need_idx, ph::AdvStatArgs& aa) {
  aa = adv_args_epochs(t.ctx, t.rb, t.perms, t.perm_seed, t.batch_size, t.n_mb);
  aa.clear_flag = t.ctx->stop_flag;  // the call's KL stop flag starts at 0 (no launch of its own: nothing reads it before the first gradient launch)
  // the split kernel reads the row records only: the materialised order (8 of the launch's 40 bytes per element) is written
  // for whoever else walks it -- the other gradient kernels, ADAP's context launch (need_idx)
  if (t.nd.split == 1 && !need_idx) aa.idx_out = aa.phys_out = nullptr;
  fill_adv_records(aa, t.ctx, t.nd, t.rb);
  // Adam's bias corrections of the call's steps ride on the same launch (one thread per minibatch): rebuilt from the device step
  // counter in every call, hence in every replay of a captured one
  aa.adam_bias = t.ctx->adam_bias;
  aa.opt_step = t.opt->step;
  aa.lr = t.hp->learning_rate;
  aa.beta1 = t.hp->adam_beta1;
  aa.beta2 = t.hp->adam_beta2;
}

// validation, workspace, stop-flag reset and the advantage statistics / minibatch order of every minibatch
int train_prepare(const char* who, TrainPlan& t, ph_ctx* ctx, const ph_spec* spec, const ph_opt_state* opt, const ph_rollout* rb,
                  const ph_ppo_hyper* hp, int n_epochs, int batch_size, const int* perms, unsigned long long perm_seed,
                  float* stats, int gemm_mode, bool need_idx = false, const ph_arch* arch = nullptr) {
  if (check_train_call(who, ctx, opt, hp, n_epochs, batch_size) || check_rb(rb)) return 1;
  t.arch = arch != nullptr;
  if (arch) {
    if (arch_resolve(ctx, spec, arch, &t.nd, &t.arch_dims)) return 1;
  } else {
    if (resolve(ctx, spec, &t.nd, true)) return 1;
    select_gemm(t.nd, gemm_mode);
  }
  t.ctx = ctx;
  t.opt = opt;
  t.rb = rb;
  t.hp = hp;
  t.perms = perms;
  t.perm_seed = perm_seed;
  t.stats = stats;
  t.n_epochs = n_epochs;
  t.batch_size = batch_size;
  t.gemm_mode = gemm_mode;
  t.N = rb->T * rb->E;
  t.n_mb = (t.N + batch_size - 1) / batch_size;
  t.P = t.nd.lay.P;
  const MbPlan big = plan_minibatch(ctx, t.nd, batch_size < t.N ? batch_size : t.N, t.arch ? &t.arch_dims : nullptr);
  if (ensure_train_ws(ctx, t.P, slab_len_of(t.nd), big.nwg, n_epochs * t.n_mb, perms ? 0 : (size_t)n_epochs * t.N,
                      (size_t)n_epochs * t.N))
    return 1;
  hipStream_t s = ctx->stream;
  if (rebuild_weight_image(ctx, t.nd, opt->params)) return 1;
  if (build_grad_pack(ctx, t.nd, rb, (size_t)n_epochs * t.N)) return 1;
  t.hb = ph::feistel_half_bits((uint32_t)t.N);
  ph::AdvStatArgs aa;
  train_adv_args(t, need_idx, aa);
  PH_HIP(ph::launch_adv_stats(aa, n_epochs * t.n_mb, s));
  return 0;
}

void fill_step_args(const TrainPlan& t, int mbi, const MbPlan& pl, ph::ReduceArgs& r, ph::AdamArgs& ad);
// ~2 s of wall_clock64 ticks (100 MHz): the bound of a wait for a workgroup that cannot be scheduled, far above any healthy one
constexpr unsigned long long STEP_WAIT_TICKS = 200000000ull;

// gradient launch of minibatch mbi = ep * n_mb + k
int train_launch_grad(const TrainPlan& t, int mbi, MbPlan* pl_out) {
  ph_ctx* ctx = t.ctx;
  const MbWalk w = minibatch_walk(ctx, t.perms, t.N, t.n_mb, t.batch_size, mbi);
  const size_t pos = (size_t)w.ep * t.N + w.start;   // of the minibatch's first row in the call's (n_epochs, N) order
  const MbPlan pl = plan_minibatch(ctx, t.nd, w.nb, t.arch ? &t.arch_dims : nullptr);
  ph::GradArgs g;
  std::memset(&g, 0, sizeof(g));
  fill_grad_args(g, t.nd, t.opt->params, t.rb, t.hp, ctx);
  g.idx = w.idx;
  g.idx_phys = ctx->perm_phys + pos;
  if (t.nd.split == 1) {
    g.rec_pi = ctx->rec_pi + pos;
    g.rec_vf = ctx->rec_vf + pos;
  }
  g.perm_n = (uint32_t)t.N;
  g.perm_hb = t.hb;
  g.perm_seed = t.perm_seed;
  g.perm_epoch = w.ep;
  g.epoch = ctx->rng_epoch;
  g.mb_start = w.start;
  g.nb = w.nb;
  g.advstats = ctx->advstats + 2 * (size_t)mbi;
  g.ntiles = pl.ntiles;
  *pl_out = pl;
  if (t.arch) PH_HIP(ph::launch_arch_grad(g, t.arch_dims, pl.nwg, t.gemm_mode, ctx->stream));
  else PH_HIP(ph::launch_ppo_grad(g, pl.nwg, t.gemm_mode, ctx->stream));
  return 0;
}

// the argument records of minibatch mbi's reduce (+ statistics, KL decision) and clip + Adam
void fill_step_args(const TrainPlan& t, int mbi, const MbPlan& pl, ph::ReduceArgs& r, ph::AdamArgs& ad) {
  ph_ctx* ctx = t.ctx;
  float* stats_out = t.stats ? t.stats + (size_t)mbi * PH_NSTAT : nullptr;
  r = reduce_args(ctx, t.hp, t.opt, t.P, slab_len_of(t.nd), t.nd.slab_map, pl.nwg, pl.nb, ctx->grad, stats_out);
  r.wide = t.alone && ctx->exclusive;
  ad = adam_args(ctx, t.hp, t.opt, t.P, slab_len_of(t.nd), stats_out, t.nd.split ? ctx->wimage : nullptr, t.nd.wimage_map);
  ad.bias = ctx->adam_bias + mbi;   // minibatch mbi takes step (the call's first) + mbi: every one before it stepped, or the call stopped
}

// slab reduction + statistics + KL decision, then clip + Adam, of the minibatch whose gradient launch returned `pl`
int train_launch_step(const TrainPlan& t, int mbi, const MbPlan& pl) {
  ph_ctx* ctx = t.ctx;
  hipStream_t s = ctx->stream;
  ph::ReduceArgs r;
  ph::AdamArgs ad;
  fill_step_args(t, mbi, pl, r, ad);
  if (t.adap) {
    const MbWalk w = minibatch_walk(ctx, t.perms, t.N, t.n_mb, t.batch_size, mbi);
    if (adap_launch(ctx, t.nd, t.opt->params, t.rb, t.adap, w.idx, w.nb, mbi, &r)) return 1;
  }
  if (step_fused_wanted(ctx, slab_len_of(t.nd), t.alone != 0)) {
    PH_HIP(ph::launch_ppo_step(r, ad, ctx->step_words, ctx->step_gen, ctx->step_gen + 1, STEP_WAIT_TICKS, s));
  } else {
    PH_HIP(ph::launch_ppo_reduce(r, s));
    PH_HIP(ph::launch_ppo_adam(ad, s));
  }
  return 0;
}

}  // namespace

namespace {
int train_run(const char* who, ph_ctx* ctx, const ph_spec* spec, const ph_opt_state* opt, const ph_rollout* rb,
              const ph_ppo_hyper* hp, int n_epochs, int batch_size, const int* perms, unsigned long long perm_seed, float* stats,
              int gemm_mode, const ph_adap_loss* adap, const ph_arch* arch = nullptr) {
  TrainPlan t;
  if (train_prepare(who, t, ctx, spec, opt, rb, hp, n_epochs, batch_size, perms, perm_seed, stats, gemm_mode, adap != nullptr, arch))
    return 1;
  if (adap && t.nd.gauss) return fail("ph_adap_train: the context term is written for the categorical heads");
  if (adap && adap_check(ctx, t.nd, adap, "ph_adap_train")) return 1;
  t.adap = adap;
  for (int mbi = 0; mbi < n_epochs * t.n_mb; ++mbi) {
    MbPlan pl;
    if (train_launch_grad(t, mbi, &pl)) return 1;
    if (train_launch_step(t, mbi, pl)) return 1;
  }
  return 0;
}
}  // namespace

int ph_ppo_train(ph_ctx* ctx, const ph_spec* spec, const ph_opt_state* opt, const ph_rollout* rb,
                 const ph_ppo_hyper* hp, int n_epochs, int batch_size, const int* perms,
                 unsigned long long perm_seed, float* stats, int gemm_mode) {
  DevGuard dev_guard(ctx);
  return train_run("ph_ppo_train", ctx, spec, opt, rb, hp, n_epochs, batch_size, perms, perm_seed, stats, gemm_mode, nullptr);
}

int ph_adap_train(ph_ctx* ctx, const ph_spec* spec, const ph_opt_state* opt, const ph_rollout* rb,
                  const ph_ppo_hyper* hp, int n_epochs, int batch_size, const int* perms,
                  unsigned long long perm_seed, float* stats, int gemm_mode, const ph_adap_loss* adap) {
  DevGuard dev_guard(ctx);
  if (!adap) return fail("ph_adap_train: null context-term description");
  return train_run("ph_adap_train", ctx, spec, opt, rb, hp, n_epochs, batch_size, perms, perm_seed, stats, gemm_mode, adap);
}

int ph_ppo_train_multi(const ph_train_call* calls, int n_calls) {
  if (!calls || n_calls <= 0) return fail("ph_ppo_train_multi: no calls");
  if (n_calls > PH_MAX_TRAIN_CALLS) return fail("ph_ppo_train_multi: too many calls");
  TrainPlan t[PH_MAX_TRAIN_CALLS];
  int total[PH_MAX_TRAIN_CALLS], longest = 0;
  for (int k = 0; k < n_calls; ++k) {
    const ph_train_call& c = calls[k];
    if (train_prepare("ph_ppo_train_multi", t[k], c.ctx, c.spec, c.opt, c.rb, c.hyper, c.n_epochs, c.batch_size, c.perms,
                      c.perm_seed, c.stats, c.gemm_mode))
      return 1;
    t[k].alone = n_calls == 1;
    if (!t[k].ctx->ev_grad) PH_HIP(hipEventCreateWithFlags(&t[k].ctx->ev_grad, hipEventDisableTiming));
    total[k] = c.n_epochs * t[k].n_mb;
    longest = total[k] > longest ? total[k] : longest;
  }
  // Round-robin over the learners, minibatch by minibatch.  Gradient launches fill the whole device, so two of them side by
  // side only slow each other down; chaining them (each waits for the previous learner's gradient launch) lets one
  // learner's small reduce / Adam launches run in the shadow of the next learner's gradient launch.
  // (Round 4 measured the alternatives on MI355X, 2 learners, whole iterations as hipGraphs: this chaining 3.62 ms; every gradient
  // launch on ONE queue with each learner's reduce / Adam on a side stream tied in by two events per minibatch 3.87 ms; NO
  // chaining at all -- one linear graph per learner, free-running, bench.py's default -- 2.74 ms.  Cross-stream edges inside a
  // graph cost far more than the overlap they arrange; the hardware's own interleaving of two independent queues wins.)
  hipEvent_t prev = nullptr;
  hipStream_t prev_stream = nullptr;
  for (int mbi = 0; mbi < longest; ++mbi) {
    for (int k = 0; k < n_calls; ++k) {
      if (mbi >= total[k]) continue;
      hipStream_t s = t[k].ctx->stream;
      if (prev && prev_stream != s) PH_HIP(hipStreamWaitEvent(s, prev, 0));
      MbPlan pl;
      if (train_launch_grad(t[k], mbi, &pl)) return 1;
      PH_HIP(hipEventRecord(t[k].ctx->ev_grad, s));
      prev = t[k].ctx->ev_grad;
      prev_stream = s;
      if (train_launch_step(t[k], mbi, pl)) return 1;
    }
  }
  return 0;
}

namespace {
int minibatch_grad_run(const char* who, ph_ctx* ctx, const ph_spec* spec, const float* params, const ph_rollout* rb,
                       const ph_ppo_hyper* hp, const int* indices, int nb, float* grad_out, float* stats_out, int gemm_mode,
                       const ph_adap_loss* adap, const ph_arch* arch = nullptr);
}  // namespace

int ph_ppo_minibatch_grad(ph_ctx* ctx, const ph_spec* spec, const float* params, const ph_rollout* rb,
                          const ph_ppo_hyper* hp, const int* indices, int nb, float* grad_out, float* stats_out,
                          int gemm_mode) {
  DevGuard dev_guard(ctx);
  return minibatch_grad_run("ph_ppo_minibatch_grad", ctx, spec, params, rb, hp, indices, nb, grad_out, stats_out, gemm_mode, nullptr);
}

int ph_adap_minibatch_grad(ph_ctx* ctx, const ph_spec* spec, const float* params, const ph_rollout* rb,
                           const ph_ppo_hyper* hp, const int* indices, int nb, float* grad_out, float* stats_out,
                           int gemm_mode, const ph_adap_loss* adap) {
  DevGuard dev_guard(ctx);
  if (!adap) return fail("ph_adap_minibatch_grad: null context-term description");
  return minibatch_grad_run("ph_adap_minibatch_grad", ctx, spec, params, rb, hp, indices, nb, grad_out, stats_out, gemm_mode, adap);
}

namespace {
int minibatch_grad_run(const char* who, ph_ctx* ctx, const ph_spec* spec, const float* params, const ph_rollout* rb,
                       const ph_ppo_hyper* hp, const int* indices, int nb, float* grad_out, float* stats_out, int gemm_mode,
                       const ph_adap_loss* adap, const ph_arch* arch) {
  if (check_minibatch_call(who, ctx, params, rb, hp, indices, nb, grad_out)) return 1;
  ph::NetDims nd;
  ph::ArchDims ad;
  if (arch) {
    if (arch_resolve(ctx, spec, arch, &nd, &ad)) return 1;
  } else {
    if (resolve(ctx, spec, &nd, adap == nullptr)) return 1;
    select_gemm(nd, gemm_mode);
  }
  const int P = nd.lay.P;
  const MbPlan pl = plan_minibatch(ctx, nd, nb, arch ? &ad : nullptr);
  if (ensure_train_ws(ctx, P, slab_len_of(nd), pl.nwg, 1, 0, (size_t)nb)) return 1;
  hipStream_t s = ctx->stream;
  PH_HIP(ph::launch_set_int(ctx->stop_flag, 0, s));
  if (rebuild_weight_image(ctx, nd, params)) return 1;
  if (build_grad_pack(ctx, nd, rb, (size_t)nb)) return 1;
  ph::AdvStatArgs aa = adv_args_minibatch(ctx, rb, indices, nb);
  fill_adv_records(aa, ctx, nd, rb);
  PH_HIP(ph::launch_adv_stats(aa, 1, s));
  ph::GradArgs g;
  std::memset(&g, 0, sizeof(g));
  fill_grad_args(g, nd, params, rb, hp, ctx);
  g.idx = indices;
  g.idx_phys = ctx->perm_phys;
  g.nb = nb;
  g.advstats = ctx->advstats;
  g.ntiles = pl.ntiles;
  if (arch) PH_HIP(ph::launch_arch_grad(g, ad, pl.nwg, gemm_mode, s));
  else PH_HIP(ph::launch_ppo_grad(g, pl.nwg, gemm_mode, s));
  ph::ReduceArgs r = reduce_args(ctx, hp, nullptr, P, slab_len_of(nd), nd.slab_map, pl.nwg, nb, grad_out, stats_out);
  if (adap) {
    if (adap_check(ctx, nd, adap, who)) return 1;
    if (adap_launch(ctx, nd, params, rb, adap, indices, nb, 0, &r)) return 1;
  }
  PH_HIP(ph::launch_ppo_reduce(r, s));
  return 0;
}
}  // namespace

// ---- MLP towers of a run-time shape (policy_kwargs net_arch; kernels: ph_arch.hip) ------------------------------------------------
int ph_arch_layout_of(const ph_spec* spec, const ph_arch* arch, ph_arch_layout* out) { return arch_layout(spec, arch, out); }

int ph_arch_lds_bytes(const ph_spec* spec, const ph_arch* arch, int* grad_bytes_out, int* grad_rows_out, int* fwd_bytes_out) {
  ph::ArchDims ad;
  ph::NetDims nd;
  if (arch_host_dims(spec, arch, &nd, &ad)) return 1;
  const int R = ph::arch_grad_rows(nd, ad);
  if (grad_bytes_out) *grad_bytes_out = (int)ph::arch_grad_lds_bytes(nd, ad, R);
  if (grad_rows_out) *grad_rows_out = R;
  if (fwd_bytes_out) *fwd_bytes_out = (int)ph::arch_fwd_lds_bytes(nd, ad);
  return 0;
}

int ph_arch_fits(const ph_spec* spec, const ph_arch* arch) {
  ph::ArchDims ad;
  ph::NetDims nd;
  if (arch_host_dims(spec, arch, &nd, &ad)) return 1;
  return arch_lds_refusal(nd, ad);
}

int ph_arch_forward(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params, const float* obs, int n,
                    const unsigned char* action_mask, const float* uniforms, const float* given_actions,
                    unsigned long long seed, unsigned long long counter, int deterministic, int* actions_i32,
                    float* actions_f32, float* values, float* log_probs, float* entropy, float* logits,
                    const ph_rollout* rb, int pos, const float* episode_start_in, const float* pending_reward, int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (!arch) return fail("null arch/layout");
  return forward_run("ph_arch_forward", ctx, spec, arch, params, obs, n, action_mask, uniforms, given_actions, seed, counter,
                     deterministic, actions_i32, actions_f32, values, log_probs, entropy, logits, rb, pos, episode_start_in,
                     pending_reward, gemm_mode);
}

int ph_arch_forward_ragged(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params, const float* obs,
                           const unsigned char* action_mask, unsigned long long seed, unsigned long long counter, int deterministic,
                           int* actions_i32, float* values, float* log_probs, const ph_rollout* rb, const int* pos_env,
                           const unsigned char* record_mask, const float* episode_start_in, int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (!arch) return fail("null arch/layout");
  return forward_ragged_run("ph_arch_forward_ragged", ctx, spec, arch, params, obs, action_mask, seed, counter, deterministic,
                            actions_i32, values, log_probs, rb, pos_env, record_mask, episode_start_in, gemm_mode);
}

int ph_arch_scripted_rollout(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params, const float* obs_seq,
                             const float* rew_seq, const float* done_seq, int n, int n_steps, const float* episode_start0,
                             unsigned long long seed, unsigned long long counter0, int* actions_i32, float* values, float* log_probs,
                             const ph_rollout* rb, int pos0, int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (!arch) return fail("null arch/layout");
  return scripted_rollout_run("ph_arch_scripted_rollout", ctx, spec, arch, params, obs_seq, rew_seq, done_seq, n, n_steps,
                              episode_start0, seed, counter0, actions_i32, values, log_probs, rb, pos0, gemm_mode);
}

int ph_arch_minibatch_grad(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const float* params, const ph_rollout* rb,
                           const ph_ppo_hyper* hp, const int* indices, int nb, float* grad_out, float* stats_out, int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (!arch) return fail("ph_arch_minibatch_grad: null arch");
  return minibatch_grad_run("ph_arch_minibatch_grad", ctx, spec, params, rb, hp, indices, nb, grad_out, stats_out, gemm_mode, nullptr,
                            arch);
}

int ph_arch_train(ph_ctx* ctx, const ph_spec* spec, const ph_arch* arch, const ph_opt_state* opt, const ph_rollout* rb,
                  const ph_ppo_hyper* hp, int n_epochs, int batch_size, const int* perms, unsigned long long perm_seed, float* stats,
                  int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (!arch) return fail("ph_arch_train: null arch");
  return train_run("ph_arch_train", ctx, spec, opt, rb, hp, n_epochs, batch_size, perms, perm_seed, stats, gemm_mode, nullptr, arch);
}

// ---- AdapPolicyMult (adap/policies.py:136-283; kernels: ph_adapmult.hip) ------------------------------------------------------
int ph_adapmult_layout_of(const ph_spec* spec, int C, ph_adapmult_layout* o) {
  if (!o) return fail("ph_adapmult_layout_of: null layout");
  ph_layout big;
  if (layout_of(spec, &big)) return 1;
  if (spec->obs.kind != PH_SPACE_BOX) return fail("AdapPolicyMult: rows are Box rows (features ++ context)");
  if (big.A != 1 || big.L > 8) return fail("AdapPolicyMult: one Discrete head of at most 8 logits");
  if (C < 1 || C > 4) return fail("AdapPolicyMult: context_size must be in [1, 4]");
  if (big.F - C < 1 || big.F - C > 64) return fail("AdapPolicyMult: 1 .. 64 features besides the context");
  const int H = PH_HIDDEN;
  o->Fo = big.F - C;
  o->C = C;
  o->L = big.L;
  int off = 0;
  o->pi_W1 = off; off += o->Fo * H;
  o->pi_b1 = off; off += H;
  o->pi_Ws = off; off += H * H * C;
  o->pi_bs = off; off += H * C;
  o->pi_W2 = off; off += H * H;
  o->pi_b2 = off; off += H;
  o->vf_W1 = off; off += o->Fo * H;
  o->vf_b1 = off; off += H;
  o->vf_Ws = off; off += H * H * C;
  o->vf_bs = off; off += H * C;
  o->vf_W2 = off; off += H * H;
  o->vf_b2 = off; off += H;
  o->act_W = off; off += H * o->L;
  o->act_b = off; off += o->L;
  o->val_W = off; off += H;
  o->val_b = off; off += 1;
  o->P = off;
  return 0;
}

namespace {
// the dense intermediates for `rows` rows of width D, carved out of one block (every array starts on a 64-float boundary)
int am_work(ph_ctx* ctx, const ph_adapmult_layout& L, int D, int rows, ph::AmWork* w) {
  const size_t H = PH_HIDDEN, C = (size_t)L.C, R = (size_t)rows;
  auto up = [](size_t n) { return (n + 63) & ~(size_t)63; };
  const size_t sizes[] = {R * H, R * H * C, R * H, R * H, R * 8, R, R * 8, R, R * H, R * H, R * H * C, R * (size_t)D,
                          R, R, R, R, R};
  size_t total = 0;
  for (size_t n : sizes) total += up(n);
  if (ensure(ctx, ctx->am_buf, ctx->am_buf_cap, total)) return 1;
  float* p = ctx->am_buf;
  float** fields[] = {&w->x, &w->xa, &w->y, &w->h, &w->z, &w->v, &w->dz, &w->dv, &w->dzh, &w->dy, &w->dza, &w->xg,
                      &w->act, &w->oldlp, &w->adv, &w->ret, &w->oldv};
  for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]); ++i) {
    *fields[i] = p;
    p += up(sizes[i]);
  }
  return 0;
}
int am_nslab(int nb) {
  const int n = (nb + 15) / 16;
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}
// PPO loss gradient of rows indices[0..nb) into ctx->slabs (am_nslab(nb) slabs of P floats, canonical order) + statistics partials,
// for the reduce record *r the caller built; with `adap` the context term's slabs and loss shares as well (the extra fields of *r).
// advstats: {mean, std} of the minibatch's advantages.
int am_minibatch(ph_ctx* ctx, const ph_adapmult_layout& L, int D, const float* params, const ph_rollout* rb, const ph_ppo_hyper* hp,
                 const int* indices, int nb, const float* advstats, const ph_adap_loss* adap, int mbi, ph::ReduceArgs* r) {
  hipStream_t s = ctx->stream;
  const int S = adap ? adap->num_state_samples : 0, Cs = adap ? adap->num_context_samples : 0;
  const int n_states = adap ? (S < nb ? S : nb) : 0;
  const int rows_max = nb > n_states * Cs ? nb : n_states * Cs;
  ph::AmWork w;
  if (am_work(ctx, L, D, rows_max, &w)) return 1;
  const int nslab = am_nslab(nb);
  ph::AmGather g;
  g.rb_obs = rb->observations;
  g.rb_act = rb->actions;
  g.rb_logp = rb->log_probs;
  g.rb_adv = rb->advantages;
  g.rb_ret = rb->returns;
  g.rb_val = rb->values;
  g.idx = indices;
  g.nb = nb;
  g.T = rb->T;
  g.E = rb->E;
  g.D = D;
  g.norm_adv = hp->normalize_advantage;
  g.advstats = advstats;
  g.xg = w.xg;
  g.act = w.act;
  g.oldlp = w.oldlp;
  g.adv = w.adv;
  g.ret = w.ret;
  g.oldv = w.oldv;
  PH_HIP(ph::launch_am_gather(g, s));
  for (int net = 0; net < 2; ++net) {
    PH_HIP(ph::am_forward_net(L, params, net, w.xg, D, nb, w, s));
    PH_HIP(ph::launch_am_loss(w, L.L, nb, *hp, ctx->statpart, nslab, net, s));
    PH_HIP(ph::am_backward_net(L, params, net, w.xg, D, nb, w, ctx->slabs, nslab, L.P, net == 0 ? L.act_W : L.val_W,
                               net == 0 ? L.act_b : L.val_b, s));
  }
  if (adap) {   // adap/util.py:97-131: n_states sampled states under Cs sampled contexts, policy net only
    const int cs = adap->context_size, extra_len = L.vf_W1 + (L.val_W - L.act_W);
    if (ensure(ctx, ctx->adap_extra, ctx->adap_extra_cap, (size_t)n_states * extra_len)) return 1;
    if (ensure(ctx, ctx->adap_loss, ctx->adap_loss_cap, (size_t)n_states)) return 1;
    ph::AmCtx a;
    std::memset(&a, 0, sizeof(a));
    a.rb_obs = rb->observations;
    a.idx = indices;
    a.nb = nb;
    a.T = rb->T;
    a.E = rb->E;
    a.D = D;
    a.ctx_size = cs;
    a.n_ctx = Cs;
    a.n_states = n_states;
    a.sampler = adap->sampler;
    a.state_idx = adap->state_idx ? adap->state_idx + (size_t)mbi * S : nullptr;
    a.contexts = adap->contexts ? adap->contexts + (size_t)mbi * Cs * cs : nullptr;
    a.seed = adap->seed;
    a.epoch = ctx->rng_epoch;
    a.mbi = (uint32_t)mbi;
    a.nb_hb = ph::feistel_half_bits((uint32_t)nb);
    a.rows = w.xg;
    a.used_state_idx = adap->used_state_idx ? adap->used_state_idx + (size_t)mbi * S : nullptr;
    a.used_contexts = adap->used_contexts ? adap->used_contexts + (size_t)mbi * Cs * cs : nullptr;
    PH_HIP(ph::launch_am_ctx_rows(a, s));
    const int R = n_states * Cs, npairs = Cs * (Cs - 1) / 2;
    PH_HIP(ph::am_forward_net(L, params, 0, w.xg, D, R, w, s));
    PH_HIP(ph::launch_am_ctx_loss(w.z, L.L, n_states, Cs, adap->context_loss_coeff / (float)(npairs * n_states), w.dz,
                                  ctx->adap_loss, s));
    // one slab per state (its Cs rows): policy-side parameters at their own offsets, the action head behind them
    PH_HIP(ph::am_backward_net(L, params, 0, w.xg, D, R, w, ctx->adap_extra, n_states, extra_len, L.vf_W1,
                               L.vf_W1 + (L.act_b - L.act_W), s));
    r->extra = ctx->adap_extra;
    r->n_extra = n_states;
    r->extra_len = extra_len;
    r->extra_cut = L.vf_W1;
    r->extra_lo = L.act_W;
    r->extra_hi = L.val_W;
    r->extra_loss = ctx->adap_loss;
    r->extra_norm = 1.0f / (float)(npairs * n_states);
    r->extra_coef = adap->context_loss_coeff;
    r->extra_loss_out = adap->context_loss ? adap->context_loss + mbi : nullptr;
  }
  return 0;
}
int am_adap_ok(const ph_adapmult_layout& L, const ph_adap_loss* ad, const char* who) {
  const std::string w(who);
  if (ad->context_size != L.C) return fail(w + ": the context term's context_size differs from the policy's");
  if (ad->num_context_samples < 2 || ad->num_context_samples > ph::ADAP_ROWS) return fail(w + ": num_context_samples must be in [2, 16]");
  if (ad->num_state_samples <= 0 || ad->num_state_samples > 256) return fail(w + ": num_state_samples must be in [1, 256]");
  if (ad->sampler < PH_CTX_L2 || ad->sampler > PH_CTX_NATURAL_NUMBERS) return fail(w + ": unknown context sampler");
  if (ad->sampler == PH_CTX_NATURAL_NUMBERS && ad->context_size != 1)
    return fail(w + ": the natural_numbers sampler draws (num, 1) contexts: context_size must be 1");
  return 0;
}
}  // namespace

int ph_adapmult_forward(ph_ctx* ctx, const ph_spec* spec, int context_size, const float* params, const float* obs, int n,
                        const unsigned char* action_mask, const float* uniforms, const float* given_actions,
                        unsigned long long seed, unsigned long long counter, int deterministic, int* actions_i32,
                        float* actions_f32, float* values, float* log_probs, float* entropy, float* logits, const ph_rollout* rb,
                        int pos, const float* episode_start_in) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!params || !obs) return fail("ph_adapmult_forward: null params/obs");
  if (n <= 0) return fail("ph_adapmult_forward: n must be positive");
  ph_adapmult_layout L;
  if (ph_adapmult_layout_of(spec, context_size, &L)) return 1;
  ph::FwdArgs a;
  if (fwd_args(a, ctx, spec, false, params, obs, n, seed, counter, actions_i32, values, log_probs)) return 1;
  fwd_eval_fields(a, action_mask, uniforms, given_actions, deterministic, actions_f32, entropy, logits);
  if (fwd_bind_row("ph_adapmult_forward", a, rb, pos, episode_start_in, nullptr)) return 1;
  ph::AmWork w;
  if (am_work(ctx, L, a.nd.D, n, &w)) return 1;
  PH_HIP(ph::am_forward_net(L, params, 0, obs, a.nd.D, n, w, ctx->stream));
  PH_HIP(ph::am_forward_net(L, params, 1, obs, a.nd.D, n, w, ctx->stream));
  PH_HIP(ph::launch_am_act(a, w.z, w.v, ctx->stream));
  return 0;
}

int ph_adapmult_minibatch_grad(ph_ctx* ctx, const ph_spec* spec, int context_size, const float* params, const ph_rollout* rb,
                               const ph_ppo_hyper* hp, const int* indices, int nb, float* grad_out, float* stats_out,
                               const ph_adap_loss* adap) {
  DevGuard dev_guard(ctx);
  // AdapPolicyMult's kernels read the parameters as plain floats: no alignment asked
  if (check_minibatch_call("ph_adapmult_minibatch_grad", ctx, params, rb, hp, indices, nb, grad_out, false)) return 1;
  ph_adapmult_layout L;
  if (ph_adapmult_layout_of(spec, context_size, &L)) return 1;
  if (adap && am_adap_ok(L, adap, "ph_adapmult_minibatch_grad")) return 1;
  const int nslab = am_nslab(nb);
  if (ensure_train_ws(ctx, L.P, L.P, nslab, 1, 0, (size_t)nb)) return 1;
  hipStream_t s = ctx->stream;
  PH_HIP(ph::launch_set_int(ctx->stop_flag, 0, s));
  PH_HIP(ph::launch_adv_stats(adv_args_minibatch(ctx, rb, indices, nb), 1, s));   // no row records: the gather kernel reads the rows
  ph::ReduceArgs r = reduce_args(ctx, hp, nullptr, L.P, L.P, nullptr, nslab, nb, grad_out, stats_out);
  if (am_minibatch(ctx, L, spec->obs.n, params, rb, hp, indices, nb, ctx->advstats, adap, 0, &r)) return 1;
  PH_HIP(ph::launch_ppo_reduce(r, s));
  return 0;
}

int ph_adapmult_train(ph_ctx* ctx, const ph_spec* spec, int context_size, const ph_opt_state* opt, const ph_rollout* rb,
                      const ph_ppo_hyper* hp, int n_epochs, int batch_size, const int* perms, unsigned long long perm_seed,
                      float* stats, const ph_adap_loss* adap) {
  DevGuard dev_guard(ctx);
  if (check_train_call("ph_adapmult_train", ctx, opt, hp, n_epochs, batch_size, false) || check_rb(rb)) return 1;
  if (!adap) return fail("ph_adapmult_train: null context-term description");
  ph_adapmult_layout L;
  if (ph_adapmult_layout_of(spec, context_size, &L)) return 1;
  if (am_adap_ok(L, adap, "ph_adapmult_train")) return 1;
  const int N = rb->T * rb->E, n_mb = (N + batch_size - 1) / batch_size;
  const int nb_max = batch_size < N ? batch_size : N;
  if (ensure_train_ws(ctx, L.P, L.P, am_nslab(nb_max), n_epochs * n_mb, perms ? 0 : (size_t)n_epochs * N, (size_t)n_epochs * N))
    return 1;
  hipStream_t s = ctx->stream;
  ph::AdvStatArgs aa = adv_args_epochs(ctx, rb, perms, perm_seed, batch_size, n_mb);   // no row records: the gather kernel reads the rows
  aa.clear_flag = ctx->stop_flag;
  PH_HIP(ph::launch_adv_stats(aa, n_epochs * n_mb, s));
  for (int mbi = 0; mbi < n_epochs * n_mb; ++mbi) {
    const MbWalk w = minibatch_walk(ctx, perms, N, n_mb, batch_size, mbi);
    float* st = stats ? stats + (size_t)mbi * PH_NSTAT : nullptr;
    ph::ReduceArgs r = reduce_args(ctx, hp, opt, L.P, L.P, nullptr, am_nslab(w.nb), w.nb, ctx->grad, st);
    if (am_minibatch(ctx, L, spec->obs.n, opt->params, rb, hp, w.idx, w.nb, ctx->advstats + 2 * (size_t)mbi, adap, mbi, &r)) return 1;
    PH_HIP(ph::launch_ppo_reduce(r, s));   // reduce, then clip + Adam: never the fused step, no weight image
    PH_HIP(ph::launch_ppo_adam(adam_args(ctx, hp, opt, L.P, L.P, st, nullptr, nullptr), s));
  }
  return 0;
}

int ph_bench_ppo_grad(ph_ctx* ctx, const ph_spec* spec, const float* params, const ph_rollout* rb,
                      const ph_ppo_hyper* hp, int batch_size, int reps, int gemm_mode, float* avg_ms_out) {
  DevGuard dev_guard(ctx);
  if (!ctx || !params || !hp || !avg_ms_out) return fail("ph_bench_ppo_grad: null argument");
  if (check_rb(rb)) return 1;
  if (batch_size <= 0 || reps <= 0) return fail("ph_bench_ppo_grad: bad sizes");
  ph::NetDims nd;
  if (resolve(ctx, spec, &nd)) return 1;
  select_gemm(nd, gemm_mode);
  const int N = rb->T * rb->E;
  const int nb = batch_size < N ? batch_size : N;
  const MbPlan pl = plan_minibatch(ctx, nd, nb);
  const int n_mb = N / nb;   // whole minibatches of one epoch's order
  if (ensure_train_ws(ctx, nd.lay.P, slab_len_of(nd), pl.nwg, n_mb, (size_t)N, (size_t)N)) return 1;
  hipStream_t s = ctx->stream;
  PH_HIP(ph::launch_set_int(ctx->stop_flag, 0, s));
  if (rebuild_weight_image(ctx, nd, params)) return 1;
  if (build_grad_pack(ctx, nd, rb, (size_t)N)) return 1;
  ph::AdvStatArgs aa = adv_args_epochs(ctx, rb, nullptr, 12345, nb, n_mb);
  aa.epoch = nullptr;   // one fixed order, whatever the RNG epoch
  if (nd.split == 1) aa.idx_out = aa.phys_out = nullptr;   // as in ph_ppo_train: the split kernel reads the row records only
  fill_adv_records(aa, ctx, nd, rb);
  PH_HIP(ph::launch_adv_stats(aa, n_mb, s));
  ph::GradArgs g;
  std::memset(&g, 0, sizeof(g));
  fill_grad_args(g, nd, params, rb, hp, ctx);
  g.perm_n = aa.perm_n;
  g.perm_hb = aa.perm_hb;
  g.perm_seed = aa.perm_seed;
  g.nb = nb;
  g.ntiles = pl.ntiles;
  auto launch = [&](int i) {
    const MbWalk w = minibatch_walk(ctx, nullptr, N, n_mb, nb, i % n_mb);
    g.idx = w.idx;
    g.idx_phys = ctx->perm_phys + w.start;
    g.mb_start = w.start;
    g.rec_pi = ctx->rec_pi ? ctx->rec_pi + w.start : nullptr;
    g.rec_vf = ctx->rec_vf ? ctx->rec_vf + w.start : nullptr;
    g.advstats = ctx->advstats + 2 * (size_t)(i % n_mb);
    return hip_rc(ph::launch_ppo_grad(g, pl.nwg, gemm_mode, s), "ph_bench_ppo_grad: launch_ppo_grad");
  };
  return time_reps(ctx, n_mb, reps, launch, avg_ms_out);   // warm: one pass over the minibatches
}

int ph_bench_gae(ph_ctx* ctx, const ph_rollout* rb, const float* last_values, const float* dones, double gamma,
                 double gae_lambda, int mode, int reps, float* avg_ms_out) {
  DevGuard dev_guard(ctx);
  if (!ctx || !last_values || !dones || !avg_ms_out) return fail("ph_bench_gae: null argument");
  if (check_rb(rb)) return 1;
  if (reps <= 0 || mode < 0 || mode > 2) return fail("ph_bench_gae: bad arguments");
  return time_reps(ctx, 1, reps, [&](int) {
    return hip_rc(ph::launch_gae(rb->rewards, rb->values, rb->episode_starts, last_values, dones, rb->advantages, rb->returns,
                                 rb->T, rb->E, gamma, gae_lambda, mode, ctx->stream), "ph_bench_gae: launch_gae");
  }, avg_ms_out);
}

int ph_bench_train_kernels(ph_ctx* ctx, const ph_spec* spec, const ph_opt_state* opt, const ph_rollout* rb,
                           const ph_ppo_hyper* hp, int n_epochs, int batch_size, int reps, int gemm_mode, float* us_out) {
  DevGuard dev_guard(ctx);
  if (!us_out) return fail("ph_bench_train_kernels: null argument");
  if (reps <= 0) return fail("ph_bench_train_kernels: reps must be positive");
  for (int i = 0; i < PH_BENCH_NKERN; ++i) us_out[i] = 0.f;
  TrainPlan t;
  if (train_prepare("ph_bench_train_kernels", t, ctx, spec, opt, rb, hp, n_epochs, batch_size, nullptr, 12345ull, nullptr, gemm_mode))
    return 1;
  hipStream_t s = ctx->stream;
  auto timed = [&](int slot, auto&& fn) -> int {   // microseconds of one fn() (0 = success) into us_out[slot]
    float ms = 0.f;
    if (time_reps(ctx, 1, reps, [&](int) { return fn(); }, &ms)) return 1;
    us_out[slot] = 1e3f * ms;
    return 0;
  };
  auto hip = [](hipError_t e) { return hip_rc(e, "ph_bench_train_kernels"); };
  if (t.nd.split) {
    if (timed(PH_BENCH_WEIGHT_IMAGE, [&] { return rebuild_weight_image(ctx, t.nd, opt->params); })) return 1;
    if (timed(PH_BENCH_OBS_PLANES, [&] { return build_grad_pack(ctx, t.nd, rb, (size_t)n_epochs * t.N); })) return 1;
  }
  ph::AdvStatArgs aa;
  train_adv_args(t, false, aa);
  if (timed(PH_BENCH_ADV_STATS, [&] { return hip(ph::launch_adv_stats(aa, n_epochs * t.n_mb, s)); })) return 1;
  MbPlan pl;
  if (train_launch_grad(t, 0, &pl)) return 1;   // slabs and partial statistics of minibatch 0 for the reduction to read
  ph::ReduceArgs r;
  ph::AdamArgs ad;
  fill_step_args(t, 0, pl, r, ad);
  r.wide = 0;
  if (timed(PH_BENCH_REDUCE, [&] { return hip(ph::launch_ppo_reduce(r, s)); })) return 1;
  r.wide = 1;
  if (timed(PH_BENCH_REDUCE_WIDE, [&] { return hip(ph::launch_ppo_reduce(r, s)); })) return 1;
  // (the reduce launches above advanced the step counter: the bias corrections again from where it stands, and the one reduce that
  // takes the step they were made for -- clip + Adam is timed as a train() call runs it)
  if (hip(ph::launch_adv_stats(aa, n_epochs * t.n_mb, s)) || hip(ph::launch_ppo_reduce(r, s))) return 1;
  if (timed(PH_BENCH_ADAM, [&] { return hip(ph::launch_ppo_adam(ad, s)); })) return 1;
  if (ctx->step_words && ctx->step_gen && ph::step_fused_fits(ph::reduce_blocks(slab_len_of(t.nd)), slab_len_of(t.nd), ctx->num_cu)) {
    if (timed(PH_BENCH_STEP_FUSED, [&] {
          return hip(ph::launch_ppo_step(r, ad, ctx->step_words, ctx->step_gen, ctx->step_gen + 1, STEP_WAIT_TICKS, s));
        }))
      return 1;
  }
  if (rb->T >= 2) {   // RolloutBuffer.add of one step (row 1 <- row 0): buffer_add_kernel
    const size_t E = (size_t)rb->E;
    if (timed(PH_BENCH_BUFFER_ADD, [&] {
          return hip(ph::launch_buffer_add(rb->observations + E * t.nd.D, rb->actions + E * t.nd.A, rb->rewards + E,
                                           rb->episode_starts + E, rb->values + E, rb->log_probs + E, rb->observations,
                                           rb->actions, rb->episode_starts, rb->values, rb->log_probs, rb->E, t.nd.D, t.nd.A, s));
        }))
      return 1;
  }
  us_out[PH_BENCH_SLAB_FLOATS] = (float)((double)pl.nwg * slab_len_of(t.nd));
  return 0;
}


// ---- ModularAlgorithm / ModularPolicy (ph_modular.hip) ---------------------------------------------------------------------
namespace {

int module_layout(int L, ph_layout* o) {   // a (Box(64), same action space) network: the partner module's parameter block
  const int H = PH_HIDDEN;
  o->D = H;
  o->F = H;
  o->A = 1;
  o->L = L;
  int off = 0;
  o->pi_W1 = off; off += H * H;
  o->pi_b1 = off; off += H;
  o->pi_W2 = off; off += H * H;
  o->pi_b2 = off; off += H;
  o->vf_W1 = off; off += H * H;
  o->vf_b1 = off; off += H;
  o->vf_W2 = off; off += H * H;
  o->vf_b2 = off; off += H;
  o->act_W = off; off += H * L;
  o->act_b = off; off += L;
  o->val_W = off; off += H;
  o->val_b = off; off += 1;
  o->P = off;
  return 0;
}

int check_modular(const ph_modular* m, const ph::NetDims& nd, const char* who) {
  const std::string w(who);
  if (!m) return fail(w + ": null ph_modular");
  if (m->num_partners < 1 || m->num_partners > PH_MOD_MAX) return fail(w + ": num_partners must be in [1, PH_MOD_MAX]");
  if (m->n_modules < 1 || m->n_modules > m->num_partners) return fail(w + ": n_modules must be in [1, num_partners]");
  for (int k = 0; k < m->num_partners; ++k)
    if (m->module_of[k] < 0 || m->module_of[k] >= m->n_modules) return fail(w + ": module_of out of range");
  if (nd.nchunk != 1 || nd.A != 1 || nd.L > 8)
    return fail(w + ": the ModularPolicy path takes observations of at most 64 features and one Discrete head of at most 8 logits");
  return 0;
}

// carve the minibatch-order activations out of one allocation
struct ModBufs {
  float *Lp, *zm, *zmod, *vm, *vk, *dzm, *dzmod, *dv, *dLa, *dLb;
};
int mod_buffers(ph_ctx* ctx, int nb, int n_mod, ModBufs* b) {
  const size_t rows = ((size_t)nb + 63) / 64 * 64;
  const size_t need = rows * (64 * 3 + 8 * 2 + 8 * 2 * (size_t)n_mod + 3);
  if (ensure(ctx, ctx->mw.act, ctx->mw.act_cap, need)) return 1;
  if (!ctx->mw.kl_sum) {
    if (ctx->capturing) return fail("first ModularPolicy call inside graph capture: call it once outside capture first");
    PH_HIP(hipMalloc((void**)&ctx->mw.kl_sum, sizeof(float)));
    PH_HIP(hipMemset(ctx->mw.kl_sum, 0, sizeof(float)));
    PH_HIP(hipMalloc((void**)&ctx->mw.scratch, (2 + PH_MOD_MAX) * sizeof(int)));
  }
  float* p = ctx->mw.act;
  b->Lp = p; p += rows * 64;
  b->dLa = p; p += rows * 64;
  b->dLb = p; p += rows * 64;
  b->zm = p; p += rows * 8;
  b->dzm = p; p += rows * 8;
  b->zmod = p; p += rows * 8 * n_mod;
  b->dzmod = p; p += rows * 8 * n_mod;
  b->vm = p; p += rows;
  b->vk = p; p += rows;
  b->dv = p; p += rows;
  return 0;
}

// slab slots of one minibatch: [main pi, main vf, module 0 pi .. module M-1 pi, trained module's vf]
int mod_slots(const ph_modular* m) { return m->n_modules + 3; }

int mod_maps(ph_ctx* ctx, const ph_spec* spec, const ph_modular* mod, const ph_layout& lay, const ph_layout& ml) {
  if (ctx->mw.maps_valid && std::memcmp(&ctx->mw.spec, spec, sizeof(ph_spec)) == 0 &&
      std::memcmp(&ctx->mw.mod, mod, sizeof(ph_modular)) == 0)
    return 0;
  if (ctx->capturing) return fail("first use of a ModularPolicy inside graph capture: call it once outside capture first");
  const int M = mod->n_modules, NS = mod_slots(mod);
  std::vector<int> h((size_t)M * NS * ph::RS_NET, -1);
  for (int k = 0; k < M; ++k) {
    int* base = h.data() + (size_t)k * NS * ph::RS_NET;
    ph::tower_slab_map(lay.F, lay.L, 1, lay.pi_W1, lay.pi_b1, lay.pi_W2, lay.pi_b2, lay.act_W, lay.act_b, base);
    ph::tower_slab_map(lay.F, lay.L, 2, lay.vf_W1, lay.vf_b1, lay.vf_W2, lay.vf_b2, lay.val_W, lay.val_b, base + ph::RS_NET);
    for (int m = 0; m < M; ++m) {
      const int o = lay.P + m * ml.P;
      ph::tower_slab_map(64, lay.L, 1, o + ml.pi_W1, o + ml.pi_b1, o + ml.pi_W2, o + ml.pi_b2, o + ml.act_W, o + ml.act_b,
                         base + (size_t)(2 + m) * ph::RS_NET);
    }
    const int o = lay.P + k * ml.P;
    ph::tower_slab_map(64, lay.L, 2, o + ml.vf_W1, o + ml.vf_b1, o + ml.vf_W2, o + ml.vf_b2, o + ml.val_W, o + ml.val_b,
                       base + (size_t)(2 + M) * ph::RS_NET);
  }
  if (ctx->mw.maps) (void)hipFree(ctx->mw.maps);
  ctx->mw.maps = nullptr;
  PH_HIP(hipMalloc((void**)&ctx->mw.maps, h.size() * sizeof(int)));
  PH_HIP(hipMemcpy(ctx->mw.maps, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
  std::memcpy(&ctx->mw.spec, spec, sizeof(ph_spec));
  std::memcpy(&ctx->mw.mod, mod, sizeof(ph_modular));
  ctx->mw.maps_valid = true;
  return 0;
}

// the towers' argument records
void tower_main(ph::TowerArgs& t, const ph::NetDims& nd, const float* params, bool policy, const float* x, int x_ld,
                const int* idx, int T, int E, int nb) {
  const ph_layout& lay = nd.lay;
  std::memset(&t, 0, sizeof(t));
  t.nb = nb;
  t.ntiles = (nb + 63) / 64;
  t.x = x;
  t.x_ld = x_ld;
  t.F = nd.F;
  t.obs_off = nd.obs_kind == PH_SPACE_BOX ? nullptr : nd.obs_off;
  t.idx = idx;
  t.T = T;
  t.E = E;
  t.W1 = params + (policy ? lay.pi_W1 : lay.vf_W1);
  t.b1 = params + (policy ? lay.pi_b1 : lay.vf_b1);
  t.W2 = params + (policy ? lay.pi_W2 : lay.vf_W2);
  t.b2 = params + (policy ? lay.pi_b2 : lay.vf_b2);
  t.hW = params + (policy ? lay.act_W : lay.val_W);
  t.hb = params + (policy ? lay.act_b : lay.val_b);
  t.head = policy ? 1 : 2;
  t.L = nd.L;
}
void tower_module(ph::TowerArgs& t, const ph_layout& lay, const ph_layout& ml, const float* params, int m, bool policy,
                  const float* latent, int nb) {
  const float* base = params + lay.P + (size_t)m * ml.P;
  std::memset(&t, 0, sizeof(t));
  t.nb = nb;
  t.ntiles = (nb + 63) / 64;
  t.x = latent;
  t.x_ld = 64;
  t.F = 64;
  t.W1 = base + (policy ? ml.pi_W1 : ml.vf_W1);
  t.b1 = base + (policy ? ml.pi_b1 : ml.vf_b1);
  t.W2 = base + (policy ? ml.pi_W2 : ml.vf_W2);
  t.b2 = base + (policy ? ml.pi_b2 : ml.vf_b2);
  t.hW = base + (policy ? ml.act_W : ml.val_W);
  t.hb = base + (policy ? ml.act_b : ml.val_b);
  t.head = policy ? 1 : 2;
  t.L = lay.L;
}

// forward of the whole DAG for `nb` rows: main towers, then every module in `mods` (policy tower; value tower too for k_mod)
int mod_forward_towers(ph_ctx* ctx, const ph::NetDims& nd, const ph_layout& ml, const float* params, const float* x, int x_ld,
                       const int* idx, int T, int E, int nb, const ModBufs& b, int n_mod, int k_mod, bool all_modules,
                       int gemm_mode, const int* stop_flag) {
  const int ntiles = (nb + 63) / 64, nwg = ntiles < ctx->num_cu ? ntiles : ctx->num_cu;
  ph::TowerLaunch L;
  std::memset(&L, 0, sizeof(L));
  L.mode = 0;
  L.stop_flag = stop_flag;
  tower_main(L.t[0], nd, params, true, x, x_ld, idx, T, E, nb);
  L.t[0].h2_out = b.Lp;
  L.t[0].head_out = b.zm;
  tower_main(L.t[1], nd, params, false, x, x_ld, idx, T, E, nb);
  L.t[1].head_out = b.vm;
  PH_HIP(ph::launch_tower(L, nwg, 2, gemm_mode, ctx->stream));
  for (int m = 0; m < n_mod; ++m) {
    if (!all_modules && m != k_mod) continue;
    tower_module(L.t[0], nd.lay, ml, params, m, true, b.Lp, nb);
    L.t[0].head_out = b.zmod + (size_t)m * nb * 8;
    int ny = 1;
    if (m == k_mod) {
      tower_module(L.t[1], nd.lay, ml, params, m, false, b.Lp, nb);
      L.t[1].head_out = b.vk;
      ny = 2;
    }
    PH_HIP(ph::launch_tower(L, nwg, ny, gemm_mode, ctx->stream));
  }
  return 0;
}

struct ModMinibatch {
  const ph_rollout* rb;
  const int* idx;
  int nb;
  const float* advstats;
  int k_mod;
  float reg_coef;
  float* stats_out;
};

// forward, loss, backward and the slab reduction of one minibatch; the gradient lands in `grad`
int mod_minibatch(ph_ctx* ctx, const ph_spec* spec, const ph_modular* mod, const ph::NetDims& nd, const ph_layout& ml,
                  const float* params, const ph_ppo_hyper* hp, const ModMinibatch& mb, float* grad, int gemm_mode) {
  const int nb = mb.nb, M = mod->n_modules, NS = mod_slots(mod);
  const int ntiles = (nb + 63) / 64, nwg = ntiles < ctx->num_cu ? ntiles : ctx->num_cu;
  ModBufs b;
  if (mod_buffers(ctx, nb, M, &b)) return 1;
  hipStream_t s = ctx->stream;
  const int T = mb.rb->T, E = mb.rb->E;
  if (mod_forward_towers(ctx, nd, ml, params, mb.rb->observations, nd.D, mb.idx, T, E, nb, b, M, mb.k_mod, true, gemm_mode,
                         ctx->stop_flag))
    return 1;
  ph::ModLossArgs la;
  std::memset(&la, 0, sizeof(la));
  la.nb = nb;
  la.idx = mb.idx;
  la.T = T;
  la.E = E;
  la.rb_act = mb.rb->actions;
  la.rb_logp = mb.rb->log_probs;
  la.rb_adv = mb.rb->advantages;
  la.rb_ret = mb.rb->returns;
  la.rb_val = mb.rb->values;
  la.advstats = mb.advstats;
  la.L = nd.L;
  la.n_mod = M;
  la.k_mod = mb.k_mod;
  la.nomain = mod->nomain;
  la.zm = b.zm;
  la.zmod = b.zmod;
  for (int m = 0; m < M; ++m) {
    int cnt = 0;
    for (int k = 0; k < mod->num_partners; ++k) cnt += mod->module_of[k] == m;
    la.weight[m] = (float)cnt / (float)mod->num_partners;
  }
  la.vm = b.vm;
  la.vk = b.vk;
  la.clip = hp->clip_range;
  la.clip_vf = hp->clip_range_vf;
  la.ent_coef = hp->ent_coef;
  la.vf_coef = hp->vf_coef;
  la.reg_coef = mb.reg_coef;
  la.dzm = b.dzm;
  la.dzmod = b.dzmod;
  la.dv = b.dv;
  la.statpart = ctx->statpart;
  la.stop_flag = ctx->stop_flag;
  PH_HIP(ph::launch_modular_loss(la, s));

  // backward: the modules first (their dL/dX is the main policy latent's gradient), the main towers last
  float* slabs = ctx->slabs;   // [nwg][NS][RS_NET]: tower slot t of workgroup w at (w * NS + t) * RS_NET
  auto slot_base = [&](int slot) { return slabs + (size_t)slot * ph::RS_NET; };
  ph::TowerLaunch L;
  std::memset(&L, 0, sizeof(L));
  L.mode = 1;
  L.stop_flag = ctx->stop_flag;
  bool first = true;
  for (int m = 0; m < M; ++m) {
    tower_module(L.t[0], nd.lay, ml, params, m, true, b.Lp, nb);
    L.t[0].dhead = b.dzmod + (size_t)m * nb * 8;
    L.t[0].dx_out = b.dLa;
    L.t[0].dx_accumulate = first ? 0 : 1;
    L.t[0].slab = slot_base(2 + m);
    L.t[0].slab_stride = NS * ph::RS_NET;
    first = false;
    int ny = 1;
    if (m == mb.k_mod) {
      tower_module(L.t[1], nd.lay, ml, params, m, false, b.Lp, nb);
      L.t[1].dhead = b.dv;
      L.t[1].dx_out = b.dLb;
      L.t[1].dx_accumulate = 0;
      L.t[1].slab = slot_base(2 + M);
      L.t[1].slab_stride = NS * ph::RS_NET;
      ny = 2;
    }
    PH_HIP(ph::launch_tower(L, nwg, ny, gemm_mode, s));
  }
  tower_main(L.t[0], nd, params, true, mb.rb->observations, nd.D, mb.idx, T, E, nb);
  L.t[0].dhead = b.dzm;
  L.t[0].ext0 = b.dLa;
  L.t[0].ext1 = b.dLb;
  L.t[0].slab = slot_base(0);
  L.t[0].slab_stride = NS * ph::RS_NET;
  tower_main(L.t[1], nd, params, false, mb.rb->observations, nd.D, mb.idx, T, E, nb);
  L.t[1].dhead = b.dv;
  L.t[1].slab = slot_base(1);
  L.t[1].slab_stride = NS * ph::RS_NET;
  PH_HIP(ph::launch_tower(L, nwg, 2, gemm_mode, s));

  ph::ReduceArgs r = reduce_args(ctx, hp, nullptr, nd.lay.P + M * ml.P, NS * ph::RS_NET,
                                 ctx->mw.maps + (size_t)mb.k_mod * NS * ph::RS_NET, nwg, nb, grad, nullptr);
  r.nstatpart = 0;              // the gradient only: the loss statistics are the finalize launch's
  r.ent_coef = r.vf_coef = 0.f;
  PH_HIP(ph::launch_ppo_reduce(r, s));
  return 0;
}

// the finalize launch of a minibatch: its loss statistics from the loss kernel's partials, the epoch's KL sum, the step counter
int mod_finalize(ph_ctx* ctx, const ph_ppo_hyper* hp, int nb, int* step, int* mod_first, int k_mod, float* stats_out,
                 float reg_coef) {
  ph::ModFinalizeArgs fa;
  std::memset(&fa, 0, sizeof(fa));
  fa.statpart = ctx->statpart;
  fa.nstatpart = (nb + 255) / 256;
  fa.nb = nb;
  fa.step = step;
  fa.mod_first = mod_first;
  fa.k_mod = k_mod;
  fa.kl_sum = ctx->mw.kl_sum;
  fa.stats_out = stats_out;
  fa.ent_coef = hp->ent_coef;
  fa.vf_coef = hp->vf_coef;
  fa.reg_coef = reg_coef;
  fa.stop_flag = ctx->stop_flag;
  PH_HIP(ph::launch_modular_finalize(fa, ctx->stream));
  return 0;
}

int mod_workspace(ph_ctx* ctx, const ph_modular* mod, int P_total, int nb_max, int n_mb_total, size_t n_idx) {
  const int ntiles = (nb_max + 63) / 64, nwg = ntiles < ctx->num_cu ? ntiles : ctx->num_cu;
  const int loss_blocks = (nb_max + 255) / 256;
  if (ensure_train_ws(ctx, P_total, mod_slots(mod) * ph::RS_NET, nwg, n_mb_total, n_idx)) return 1;
  if (ensure(ctx, ctx->statpart, ctx->statpart_cap, (size_t)(loss_blocks > 2 * nwg ? loss_blocks : 2 * nwg) * ph::NSTATP))
    return 1;
  return 0;
}
}  // namespace

int ph_modular_layout(const ph_spec* spec, const ph_modular* mod, ph_layout* main_out, ph_layout* module_out, int* p_total_out) {
  if (!spec || !mod) return fail("ph_modular_layout: null argument");
  ph_layout lay, ml;
  if (layout_of(spec, &lay)) return 1;
  module_layout(lay.L, &ml);
  if (mod->n_modules < 1 || mod->n_modules > PH_MOD_MAX) return fail("ph_modular_layout: n_modules must be in [1, PH_MOD_MAX]");
  if (main_out) *main_out = lay;
  if (module_out) *module_out = ml;
  if (p_total_out) *p_total_out = lay.P + mod->n_modules * ml.P;
  return 0;
}

int ph_modular_forward(ph_ctx* ctx, const ph_spec* spec, const ph_modular* mod, const float* params, int partner_idx,
                       const float* obs, int n, const unsigned char* action_mask, const float* uniforms,
                       const float* given_actions, unsigned long long seed, unsigned long long counter, int deterministic,
                       int* actions_i32, float* actions_f32, float* values, float* log_probs, float* entropy,
                       float* logits_main, float* logits_partner, const ph_rollout* rb, int pos,
                       const float* episode_start_in, const float* pending_reward, int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!params || !obs) return fail("ph_modular_forward: null params/obs");
  if ((uintptr_t)params % 16 != 0) return fail("ph_modular_forward: params must be 16-byte aligned");
  if (n <= 0) return fail("ph_modular_forward: n must be positive");
  ph::FwdArgs a;
  if (fwd_args(a, ctx, spec, false, params, obs, n, seed, counter, actions_i32, values, log_probs)) return 1;
  if (check_modular(mod, a.nd, "ph_modular_forward")) return 1;
  if (partner_idx < 0 || partner_idx >= mod->num_partners) return fail("ph_modular_forward: partner_idx out of range");
  ph_layout ml;
  module_layout(a.nd.L, &ml);
  const int k_mod = mod->module_of[partner_idx];
  ModBufs b;
  if (mod_buffers(ctx, n, mod->n_modules, &b)) return 1;
  if (mod_forward_towers(ctx, a.nd, ml, params, obs, a.nd.D, nullptr, 0, 0, n, b, mod->n_modules, k_mod, false, gemm_mode,
                         nullptr))
    return 1;
  fwd_eval_fields(a, action_mask, uniforms, given_actions, deterministic, actions_f32, entropy, nullptr);   // logits: its own two
  if (fwd_bind_row("ph_modular_forward", a, rb, pos, episode_start_in, pending_reward)) return 1;
  PH_HIP(ph::launch_modular_act(a, b.zm, b.zmod + (size_t)k_mod * n * 8, b.vm, b.vk, mod->nomain, logits_main, logits_partner,
                                ctx->stream));
  return 0;
}

int ph_modular_minibatch_grad(ph_ctx* ctx, const ph_spec* spec, const ph_modular* mod, const float* params, int partner_idx,
                              const ph_rollout* rb, const ph_ppo_hyper* hp, const int* indices, int nb, float marginal_reg_coef,
                              float* grad_out, float* stats_out, int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (check_minibatch_call("ph_modular_minibatch_grad", ctx, params, rb, hp, indices, nb, grad_out)) return 1;
  ph::NetDims nd;
  if (resolve(ctx, spec, &nd)) return 1;
  if (check_modular(mod, nd, "ph_modular_minibatch_grad")) return 1;
  if (partner_idx < 0 || partner_idx >= mod->num_partners) return fail("ph_modular_minibatch_grad: partner_idx out of range");
  ph_layout ml;
  module_layout(nd.L, &ml);
  const int P_total = nd.lay.P + mod->n_modules * ml.P;
  if (mod_workspace(ctx, mod, P_total, nb, 1, 0)) return 1;
  if (mod_maps(ctx, spec, mod, nd.lay, ml)) return 1;
  hipStream_t s = ctx->stream;
  PH_HIP(ph::launch_set_int(ctx->stop_flag, 0, s));
  ph::AdvStatArgs aa = adv_args_minibatch(ctx, rb, indices, nb);
  aa.phys_out = nullptr;   // the towers gather their rows through the env-major indices
  PH_HIP(ph::launch_adv_stats(aa, 1, s));
  PH_HIP(hipMemsetAsync(grad_out, 0, (size_t)P_total * sizeof(float), s));
  const ModMinibatch mb{rb, indices, nb, ctx->advstats, mod->module_of[partner_idx], marginal_reg_coef, stats_out};
  if (mod_minibatch(ctx, spec, mod, nd, ml, params, hp, mb, grad_out, gemm_mode)) return 1;
  if (stats_out) {   // statistics without touching any optimizer state: a scratch step counter / first-use table
    PH_HIP(hipMemsetAsync(ctx->mw.scratch, 0, (2 + PH_MOD_MAX) * sizeof(int), s));
    if (mod_finalize(ctx, hp, nb, ctx->mw.scratch, ctx->mw.scratch + 1, 0, stats_out, marginal_reg_coef)) return 1;
  }
  return 0;
}

int ph_modular_train(ph_ctx* ctx, const ph_spec* spec, const ph_modular* mod, const ph_opt_state* opt, int* mod_first,
                     const ph_rollout* rbs, const ph_ppo_hyper* hp, int n_epochs, int batch_size, const int* perms,
                     unsigned long long perm_seed, float* stats, float marginal_reg_coef, int gemm_mode) {
  DevGuard dev_guard(ctx);
  if (check_train_call("ph_modular_train", ctx, opt, hp, n_epochs, batch_size)) return 1;
  if (!mod_first) return fail("ph_modular_train: null optimizer state");
  if (!rbs) return fail("ph_modular_train: null argument");
  ph::NetDims nd;
  if (resolve(ctx, spec, &nd)) return 1;
  if (check_modular(mod, nd, "ph_modular_train")) return 1;
  ph_layout ml;
  module_layout(nd.L, &ml);
  const int M = mod->n_modules, P_total = nd.lay.P + M * ml.P;
  for (int k = 0; k < mod->num_partners; ++k) {
    if (check_rb(&rbs[k])) return 1;
    if (rbs[k].T != rbs[0].T || rbs[k].E != rbs[0].E) return fail("ph_modular_train: the partners' rollout buffers must have one shape");
  }
  const int N = rbs[0].T * rbs[0].E;
  const int n_mb = (N + batch_size - 1) / batch_size;
  const int nb_max = batch_size < N ? batch_size : N;
  if (mod_workspace(ctx, mod, P_total, nb_max, n_epochs * n_mb, perms ? 0 : (size_t)n_epochs * N)) return 1;
  if (mod_maps(ctx, spec, mod, nd.lay, ml)) return 1;
  {
    ModBufs probe;
    if (mod_buffers(ctx, nb_max, M, &probe)) return 1;
  }
  hipStream_t s = ctx->stream;
  for (int k = 0; k < mod->num_partners; ++k) {
    const ph_rollout* rb = &rbs[k];
    const int k_mod = mod->module_of[k];
    PH_HIP(ph::launch_set_int(ctx->stop_flag, 0, s));
    PH_HIP(hipMemsetAsync(ctx->mw.kl_sum, 0, sizeof(float), s));
    const int* perms_k = perms ? perms + (size_t)k * n_epochs * N : nullptr;
    const unsigned long long seed_k = perm_seed + (unsigned long long)k * 0x9E3779B97F4A7C15ull;   // an order per partner
    ph::AdvStatArgs aa = adv_args_epochs(ctx, rb, perms_k, seed_k, batch_size, n_mb);
    aa.phys_out = nullptr;   // the towers gather their rows through the env-major indices
    PH_HIP(ph::launch_adv_stats(aa, n_epochs * n_mb, s));
    for (int ep = 0; ep < n_epochs; ++ep) {
      for (int j = 0; j < n_mb; ++j) {
        const int mbi = ep * n_mb + j;
        const MbWalk w = minibatch_walk(ctx, perms_k, N, n_mb, batch_size, mbi);
        float* st = stats ? stats + ((size_t)k * n_epochs * n_mb + mbi) * PH_NSTAT : nullptr;
        const ModMinibatch mb{rb, w.idx, w.nb, ctx->advstats + 2 * (size_t)mbi, k_mod, marginal_reg_coef, st};
        if (mod_minibatch(ctx, spec, mod, nd, ml, opt->params, hp, mb, ctx->grad, gemm_mode)) return 1;
        if (mod_finalize(ctx, hp, w.nb, opt->step, mod_first, k_mod, st, marginal_reg_coef)) return 1;
        ph::ModAdamArgs ad;
        std::memset(&ad, 0, sizeof(ad));
        ad.params = opt->params;
        ad.m = opt->adam_m;
        ad.v = opt->adam_v;
        ad.grad = ctx->grad;
        ad.blocksq = ctx->blocksq;
        ad.nblk = ph::reduce_blocks(mod_slots(mod) * ph::RS_NET);
        ad.P = P_total;
        ad.step = opt->step;
        ad.lr = hp->learning_rate;
        ad.beta1 = hp->adam_beta1;
        ad.beta2 = hp->adam_beta2;
        ad.eps = hp->adam_eps;
        ad.max_norm = hp->max_grad_norm;
        ad.stats_out = st;
        ad.n_mod = M;
        ad.k_mod = k_mod;
        ad.n_seg = 2 * M;
        for (int m = 0; m < M; ++m) {
          const int o = nd.lay.P + m * ml.P;
          ad.seg_lo[2 * m] = o + ml.vf_W1;
          ad.seg_hi[2 * m] = o + ml.act_W;
          ad.seg_mod[2 * m] = m;
          ad.seg_lo[2 * m + 1] = o + ml.val_W;
          ad.seg_hi[2 * m + 1] = o + ml.P;
          ad.seg_mod[2 * m + 1] = m;
        }
        ad.mod_first = mod_first;
        ad.stop_flag = ctx->stop_flag;
        PH_HIP(ph::launch_modular_adam(ad, s));
      }
      PH_HIP(ph::launch_modular_epoch_end(ctx->mw.kl_sum, n_mb, hp->target_kl, ctx->stop_flag, s));
    }
  }
  PH_HIP(ph::launch_set_int(ctx->stop_flag, 0, s));
  return 0;
}

// ---- behavioural cloning on the shared 32-32 policy ----
int ph_bc_layout_of(const ph_spec* spec, ph_bc_layout* o) {
  ph_layout big;
  if (!o) return fail("null layout");
  if (layout_of(spec, &big)) return 1;
  const int H = PH_BC_HIDDEN;
  o->D = big.D;
  o->F = big.F;
  o->A = big.A;
  o->L = big.L;
  int off = 0;
  o->W1 = off; off += big.F * H;
  o->b1 = off; off += H;
  o->W2 = off; off += H * H;
  o->b2 = off; off += H;
  o->act_W = off; off += H * big.L;
  o->act_b = off; off += big.L;
  o->val_W = off; off += H;
  o->val_b = off; off += 1;
  o->P = off;
  return 0;
}

int ph_bc_train_path(const ph_spec* spec, int* out) {
  if (!out) return fail("ph_bc_train_path: null out");
  ph_bc_layout lay;
  if (ph_bc_layout_of(spec, &lay)) return 1;
  if (spec->act.kind != PH_SPACE_DISCRETE) return fail("ph_bc_train_path: BC clones categorical actions");
  *out = ph::bc_train_path(lay.D, lay.F, lay.A, lay.L, lay.P);
  return 0;
}

int ph_bc_forward(ph_ctx* ctx, const ph_spec* spec, const float* params, const float* obs, int n,
                  const unsigned char* action_mask, const float* uniforms, const float* given_actions,
                  unsigned long long seed, unsigned long long counter, int deterministic, int* actions_i32, float* values,
                  float* log_probs, float* entropy, float* logits) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!params || !obs || n <= 0) return fail("ph_bc_forward: bad argument");
  ph::NetDims nd;
  if (resolve(ctx, spec, &nd)) return 1;
  ph_bc_layout lay;
  if (ph_bc_layout_of(spec, &lay)) return 1;
  if (ph::bc_forward_lds_bytes(lay.P) > 160 * 1024) return fail("ph_bc_forward: policy too large for the LDS-resident forward");
  PH_HIP(ph::launch_bc_forward(nd, lay, params, obs, n, action_mask, uniforms, given_actions, seed, counter, deterministic,
                               actions_i32, values, log_probs, entropy, logits, ctx->stream));
  return 0;
}

int ph_bc_train(ph_ctx* ctx, const ph_spec* spec, const ph_opt_state* opt, const float* obs, const float* acts,
                const int* order, int N, int batch_size, int n_epochs, int max_batches, const ph_bc_hyper* hyper,
                float* stats) {
  DevGuard dev_guard(ctx);
  if (!ctx) return fail("null ctx");
  if (!opt || !opt->params || !opt->adam_m || !opt->adam_v || !opt->step) return fail("ph_bc_train: null optimizer state");
  if (!obs || !acts || !order || !hyper) return fail("ph_bc_train: null argument");
  if (N <= 0 || batch_size <= 0 || n_epochs <= 0) return fail("ph_bc_train: N, batch_size and n_epochs must be positive");
  ph::NetDims nd;
  if (resolve(ctx, spec, &nd)) return 1;
  ph_bc_layout lay;
  if (ph_bc_layout_of(spec, &lay)) return 1;
  if (ph::bc_train_path(nd.D, nd.F, nd.A, nd.L, lay.P) == 0) return fail("ph_bc_train: working set exceeds the CU's 160 KiB of LDS");
  PH_HIP(ph::launch_bc_train(nd, lay, opt->params, opt->adam_m, opt->adam_v, opt->step, obs, acts, order, N, batch_size,
                             n_epochs, max_batches, *hyper, stats, ctx->stream));
  return 0;
}

int ph_feistel_indices(int n, unsigned long long perm_seed, int epoch, int start, int count, int* out) {
  if (!out) return fail("ph_feistel_indices: null out");
  if (n <= 0 || start < 0 || count < 0 || (long long)start + count > n) return fail("ph_feistel_indices: bad range");
  const uint32_t hb = ph::feistel_half_bits((uint32_t)n);
  const uint64_t key = ph::epoch_key(perm_seed, epoch);
  for (int i = 0; i < count; ++i) out[i] = (int)ph::feistel_perm((uint32_t)(start + i), (uint32_t)n, hb, key);
  return 0;
}

}  // extern "C"
