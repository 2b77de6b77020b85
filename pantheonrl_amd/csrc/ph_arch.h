// MLP towers of a run-time shape (policy_kwargs net_arch): records and launcher prototypes shared by ph_arch.hip and ph_abi.hip.
#pragma once
#include "ph_launch.h"

namespace ph {

// the arch resolved for kernels.  Kernel-argument arrays are only ever read through pick3 (constant indices): a dynamically indexed
// by-value argument sends the whole argument block to scratch.
struct ArchDims {
  int nl;          // layers of either tower (1..PH_ARCH_MAX_LAYERS)
  int w[3];        // their widths (unused entries 0)
  ph_arch_layout lay;
};
// (On the device the three values pass through an empty asm first: left alone, the compiler folds the select over three loads
// into one load at a selected ADDRESS and parks the kernel-argument array in scratch for it.)
__host__ __device__ inline int pick3(const int (&v)[3], int l) {
  int a = v[0], b = v[1], c = v[2];
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(a), "+s"(b), "+s"(c));
#endif
  return l == 0 ? a : (l == 1 ? b : c);
}

// LDS carve of the tower kernels (floats from the start of dynamic LDS), the same function on both sides of the launch.
// R rows per tile; a staged weight block is 64 x NBW (forward) or NBW x 64 (back-propagation), NBW = 32 * (128 / R): four 32x32
// output tiles per staged block, one per wave.
struct ArchLds {
  int act[3];      // H_l [R][w_l + 1]: activations of layer l, later dZ_l in place
  int bufx;        // [R][LDH] X chunk (layer 1 and dW1)  |  OUT [R][Lp + 1] (head phases): disjoint lifetimes
  int wst;         // staged weight block
  int bias;        // [3][256]
  int bos;         // act_b [Lp] (policy) | val_W [w_n] (value)
  int radv, rold, rdv;   // [R] each
  int red;         // [NSTATP * 4]
  int rowphys;     // [R] int
  int feat;        // [R][D] int (one-hot observations)
  int fcomp;       // [nchunk * 64] int (one-hot observations)
  int total;       // floats
};
__host__ __device__ inline int arch_nbw(int R) { return 32 * (128 / R); }
__host__ __device__ inline ArchLds arch_lds(const ArchDims& ad, int R, int onehot_D, int nchunk) {
  ArchLds L;
  int o = 0;
  for (int l = 0; l < 3; ++l) {
    L.act[l] = o;
    if (l < ad.nl) o += R * (pick3(ad.w, l) + 1);
  }
  L.bufx = o; o += R * (HID + 1);
  const int nbw = arch_nbw(R);
  L.wst = o; o += (64 * (nbw + 1) > nbw * 65) ? 64 * (nbw + 1) : nbw * 65;
  L.bias = o; o += 3 * PH_ARCH_MAX_WIDTH;
  L.bos = o; o += PH_ARCH_MAX_WIDTH;
  L.radv = o; o += R;
  L.rold = o; o += R;
  L.rdv = o; o += R;
  L.red = o; o += NSTATP * 4;
  L.rowphys = o; o += R;
  L.feat = o; o += R * onehot_D;
  L.fcomp = o; o += onehot_D ? nchunk * HID : 0;
  L.total = o;
  return L;
}

constexpr size_t ARCH_LDS_MAX = 160 * 1024;            // the CU's LDS
constexpr size_t ARCH_SLAB_CAP_BYTES = 256u << 20;     // gradient slabs of one launch: at most this much workspace
constexpr int ARCH_FWD_ROWS = 32;

// tile height of the gradient launch: 64 rows where the carve fits the CU's LDS, else 32
int arch_grad_rows(const NetDims& nd, const ArchDims& ad);
size_t arch_grad_lds_bytes(const NetDims& nd, const ArchDims& ad, int R);
size_t arch_fwd_lds_bytes(const NetDims& nd, const ArchDims& ad);
// tiles and workgroups per net of a minibatch of nb rows (slab cap and residency applied)
void arch_grad_plan(const NetDims& nd, const ArchDims& ad, int nb, int num_cu, int* ntiles, int* nwg);
hipError_t launch_arch_grad(const GradArgs& a, const ArchDims& ad, int nwg, int gemm_mode, hipStream_t s);
hipError_t launch_arch_fwd(const FwdArgs& a, const ArchDims& ad, int gemm_mode, hipStream_t s);
// sc.n_steps forwards against a scripted environment in one launch (tower_rollout_kernel)
hipError_t launch_arch_rollout(const FwdArgs& a, const ArchDims& ad, const ScriptedSteps& sc, int gemm_mode, hipStream_t s);

}  // namespace ph
