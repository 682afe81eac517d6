// index_build.hip — K1 of the GICP hot path: the spatial index of a cloud.
//
//   K1 index build      k_pack_bbox, k_bbox_final, k_morton, k_gather,
//                       k_key_dir / k_key_big / k_key_fine (key directory),
//                       k_leaf_soa_boxes, k_level_boxes   (radix sort: hipcub, cloud.hip)
// Compiled with -ffp-contract=off, like every stage file: fp32 distance /
// transform arithmetic must not be contracted into FMAs so that
// correspondences equal the oracle's.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "gicp_types.hpp"
#include "search.hpp"
#include "launch.hpp"
#include "launch_util.hpp"

namespace ddlo {

// ============================================================================
// K1: cloud packing, bbox, Morton keys, hierarchy boxes
// ============================================================================
__global__ __launch_bounds__(256) void k_pack_bbox(const unsigned char* __restrict__ raw, size_t stride, int n,
                                                   float4* __restrict__ out, float* __restrict__ partial,
                                                   int* __restrict__ nonfinite) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  bool ok = false;
  if (i < n) {
    const float* p = reinterpret_cast<const float*>(raw + (size_t)i * stride);
    x = p[0];
    y = p[1];
    z = p[2];
    ok = isfinite(x) && isfinite(y) && isfinite(z);
    out[i] = make_float4(x, y, z, __int_as_float(i));
  }
  // one flag write per wavefront holding a non-finite point (one word takes ~88 atomics per us)
  const unsigned long long bad = __ballot(i < n && !ok);
  if (bad && __lane_id() == (unsigned)__builtin_ctzll(bad)) atomicOr(nonfinite, 1);
  __shared__ float red[6][4];
  float v[6] = {ok ? x : INFINITY, ok ? y : INFINITY, ok ? z : INFINITY,
                ok ? x : -INFINITY, ok ? y : -INFINITY, ok ? z : -INFINITY};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    v[a] = wave_min(v[a]);
    v[a + 3] = wave_max(v[a + 3]);
  }
  const int w = threadIdx.x >> 6;
  if (lane_id() == 0)
    for (int a = 0; a < 6; ++a) red[a][w] = v[a];
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float r = red[a][0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r = a < 3 ? fminf(r, red[a][k]) : fmaxf(r, red[a][k]);
    partial[blockIdx.x * 6 + a] = r;
  }
}

__global__ __launch_bounds__(256) void k_bbox_final(const float* __restrict__ partial, int nparts,
                                                    float* __restrict__ quant) {
  // one block of 256 threads: strided partial min/max, then wave + LDS reduce
  __shared__ float red[6][4];
  __shared__ float bb[6];
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int k = threadIdx.x; k < nparts; k += blockDim.x) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = fminf(v[a], partial[k * 6 + a]);
      v[a + 3] = fmaxf(v[a + 3], partial[k * 6 + a + 3]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    v[a] = wave_min(v[a]);
    v[a + 3] = wave_max(v[a + 3]);
  }
  if (lane_id() == 0)
    for (int a = 0; a < 6; ++a) red[a][threadIdx.x >> 6] = v[a];
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float r = red[a][0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = a < 3 ? fminf(r, red[a][w]) : fmaxf(r, red[a][w]);
    bb[a] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float ext = fmaxf(fmaxf(bb[3] - bb[0], bb[4] - bb[1]), bb[5] - bb[2]);
    quant[0] = bb[0];
    quant[1] = bb[1];
    quant[2] = bb[2];
    quant[3] = ext > 0.f ? 2097151.f / ext : 1.f;
    quant[4] = bb[3];
    quant[5] = bb[4];
    quant[6] = bb[5];
  }
}

__global__ __launch_bounds__(256) void k_morton(const float4* __restrict__ pts, int n, const float* __restrict__ quant,
                                                unsigned long long* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  keys[i] = morton_key(p.x, p.y, p.z, quant);
  vals[i] = i;
}

// Sorted gather; positions [n, npad) get far sentinels (squared distance
// ~3e36 to any real point) so leaf scans never need a bound check.
constexpr float kFar = 1e18f;
__global__ __launch_bounds__(256) void k_gather(const float4* __restrict__ raw, const int* __restrict__ perm, int n,
                                                int npad, float4* __restrict__ sorted, int* __restrict__ inv_perm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad) return;
  if (i >= n) {
    sorted[i] = make_float4(kFar, kFar, kFar, __int_as_float(-1));
    return;
  }
  const int o = perm[i];
  sorted[i] = raw[o];
  inv_perm[o] = i;
}

// Key directory (search.hpp dir_range): thread i of the sorted keys fills
// the prefixes in (prefix(i - 1), prefix(i)] with i; the last thread also
// fills the prefixes past the largest key with n.
__global__ __launch_bounds__(256) void k_key_dir(const unsigned long long* __restrict__ keys, int n, int* __restrict__ dir) {
  // dir[p] = first sorted position whose top kDirBits Morton bits are >= p
  // (p in [0, 2^kDirBits]); one thread per entry, a lower-bound search each,
  // so empty stretches of the Morton space cost no serial fill
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > (1 << kDirBits)) return;
  constexpr int sh = 63 - kDirBits;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long)(keys[mid] >> sh) < (long)p) lo = mid + 1;
    else hi = mid;
  }
  dir[p] = lo;
}

// Fine directory: a bucket of more than kFineMin keys (and fewer than 2^16)
// takes a slot, and lane f of the wavefront refining it stores the lower
// bound of refinement f (the next kFineBits Morton bits) relative to the
// bucket start.  Two launches: k_key_big (a lane per bucket) assigns the
// slots and leaves each slot's bucket in the slot's first int; k_key_fine (a
// wavefront per possible slot) refines.  A wavefront per bucket spent ~30 us
// per cloud launching 2^18 mostly idle wavefronts.  Slot order depends on
// scheduling, the contents do not.
__global__ __launch_bounds__(256) void k_key_big(int* __restrict__ dir) {
  const int c = (int)blockIdx.x * blockDim.x + (int)threadIdx.x;
  if (c >= (1 << kDirBits)) return;
  int* const ctr = dir + (1 << kDirBits) + 1;
  int* const fslot = ctr + 1;
  unsigned short* const fine = reinterpret_cast<unsigned short*>(fslot + (1 << kDirBits));
  const int nk = dir[c + 1] - dir[c];
  const bool big = nk > kFineMin && nk <= 65535;
  const unsigned long long m = __ballot(big);
  int base = 0;
  if (m) {
    if (lane_id() == __builtin_ctzll(m)) base = atomicAdd(ctr, __popcll(m));
    base = __shfl(base, __builtin_ctzll(m));
  }
  int slot = -1;
  if (big) {
    slot = base + __popcll(m & ((1ull << lane_id()) - 1));
    reinterpret_cast<int*>(fine + ((size_t)slot << kFineBits))[0] = c;
  }
  fslot[c] = slot;
}

__global__ __launch_bounds__(256) void k_key_fine(const unsigned long long* __restrict__ keys, int* __restrict__ dir) {
  const int slot = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  const int lane = lane_id();
  int* const ctr = dir + (1 << kDirBits) + 1;
  if (slot >= __builtin_amdgcn_readfirstlane(*ctr)) return;
  int* const fslot = ctr + 1;
  unsigned short* const fine = reinterpret_cast<unsigned short*>(fslot + (1 << kDirBits));
  const int c = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(fine + ((size_t)slot << kFineBits))[0]);
  const int lo = dir[c], hi = dir[c + 1];
  constexpr int sh = 63 - kDirBits - kFineBits;
  const unsigned long long want = ((unsigned long long)c << kFineBits) | (unsigned long long)lane;
  int a = lo, b = hi;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if ((keys[mid] >> sh) < want) a = mid + 1;
    else b = mid;
  }
  __builtin_amdgcn_wave_barrier();   // every lane has read the slot's bucket id before lanes 0-1 overwrite it
  fine[((size_t)slot << kFineBits) + lane] = (unsigned short)(a - lo);
}

// Per-leaf SoA copy of the sorted points (leaf l = x[32], y[32], z[32], so
// that a lane's 8 consecutive coordinates are two 16-B loads per axis and
// pairs of them feed the packed-math distance directly, k_nn_scan) and each
// leaf's box over its real points, in one pass: thread = sorted position,
// 32 threads per leaf (8 leaves per block).
__global__ __launch_bounds__(256) void k_leaf_soa_boxes(const float4* __restrict__ pts, int n, int nleaves,
                                                        float* __restrict__ soa, float4* __restrict__ lo,
                                                        float4* __restrict__ hi) {
  const int leaf = blockIdx.x * 8 + (threadIdx.x >> 5);
  const int sub = threadIdx.x & 31;
  const int p = leaf * kLeafSize + sub;
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (leaf < nleaves) {   // the sentinel-padded positions of the last leaf are copied too
    const float4 q = pts[p];
    float* o = soa + (size_t)leaf * 3 * kLeafSize;
    o[sub] = q.x;
    o[kLeafSize + sub] = q.y;
    o[2 * kLeafSize + sub] = q.z;
    if (p < n) {
      v[0] = v[3] = q.x;
      v[1] = v[4] = q.y;
      v[2] = v[5] = q.z;
    }
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = fminf(v[a], __shfl_xor(v[a], m));
      v[a + 3] = fmaxf(v[a + 3], __shfl_xor(v[a + 3], m));
    }
  }
  if (sub == 0 && leaf < nleaves) {
    lo[leaf] = make_float4(v[0], v[1], v[2], 0.f);
    hi[leaf] = make_float4(v[3], v[4], v[5], 0.f);
  }
}

// one wavefront per parent node, lane = child
__global__ __launch_bounds__(256) void k_level_boxes(const float4* __restrict__ clo, const float4* __restrict__ chi,
                                                     int nchild, int nparent, float4* __restrict__ plo,
                                                     float4* __restrict__ phi) {
  const int parent = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int c = parent * kFanout + lane_id();
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (parent < nparent && c < nchild) {
    const float4 a = clo[c], b = chi[c];
    v[0] = a.x; v[1] = a.y; v[2] = a.z;
    v[3] = b.x; v[4] = b.y; v[5] = b.z;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    v[a] = wave_min(v[a]);
    v[a + 3] = wave_max(v[a + 3]);
  }
  if (lane_id() == 0 && parent < nparent) {
    plo[parent] = make_float4(v[0], v[1], v[2], 0.f);
    phi[parent] = make_float4(v[3], v[4], v[5], 0.f);
  }
}

void launch_pack_bbox(hipStream_t s, const unsigned char* raw, size_t stride, int n, float4* out, float* partial,
                      int* nonfinite, int nblocks) {
  k_pack_bbox<<<nblocks, 256, 0, s>>>(raw, stride, n, out, partial, nonfinite);
}
void launch_bbox_final(hipStream_t s, const float* partial, int nparts, float* quant) {
  k_bbox_final<<<1, 256, 0, s>>>(partial, nparts, quant);
}
void launch_morton(hipStream_t s, const float4* pts, int n, const float* quant, unsigned long long* keys, int* vals) {
  k_morton<<<cdiv(n, 256), 256, 0, s>>>(pts, n, quant, keys, vals);
}
void launch_gather(hipStream_t s, const float4* raw, const int* perm, int n, int npad, float4* sorted, int* inv_perm) {
  k_gather<<<cdiv(npad, 256), 256, 0, s>>>(raw, perm, n, npad, sorted, inv_perm);
}
void launch_key_dir(hipStream_t s, const unsigned long long* keys, int n, int* dir) {
  k_key_dir<<<cdiv((1 << kDirBits) + 1, 256), 256, 0, s>>>(keys, n, dir);
  (void)hipMemsetAsync(dir + (1 << kDirBits) + 1, 0, sizeof(int), s);   // fine-slot counter
  k_key_big<<<(1 << kDirBits) / 256, 256, 0, s>>>(dir);
  const long max_slots = (long)n / (kFineMin + 1) + 1;   // (fine_dir_ints)
  k_key_fine<<<cdiv(max_slots, 4), 256, 0, s>>>(keys, dir);
}
void launch_leaf_soa_boxes(hipStream_t s, const float4* pts, int n, int nleaves, float* soa, float4* lo, float4* hi) {
  k_leaf_soa_boxes<<<cdiv(nleaves, 8), 256, 0, s>>>(pts, n, nleaves, soa, lo, hi);
}
void launch_level_boxes(hipStream_t s, const float4* clo, const float4* chi, int nchild, int nparent, float4* plo,
                        float4* phi) {
  k_level_boxes<<<cdiv(nparent, 4), 256, 0, s>>>(clo, chi, nchild, nparent, plo, phi);
}

}  // namespace ddlo
