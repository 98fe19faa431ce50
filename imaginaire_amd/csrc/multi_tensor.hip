// k4 / k5: multi-tensor optimizer and model-averaging kernels.
//
// One launch covers every parameter tensor of a network: the host builds a
// device-resident table {pointers, numel} plus a block map (tensor id, chunk
// offset) once per distinct tensor list (cached by pointer signature, so the
// steady state costs no host work beyond a hash and is hipGraph-capturable),
// and each workgroup streams one 16-byte-vectorised chunk.
//
//   mt_adam     : Adam / AdamW (reference FusedAdam, utils/trainer.py:271-281)
//                 fp32 master params, fp32 or bf16 grads, optional bf16 shadow
//                 copy of the updated weights written in the same pass.
//   mt_sn_sigma : σ_i = u_iᵀ W_i v_i for every spectral-normalised weight
//                 (reference ModelAverage.sn_compute_weight, model_average.py:183-197)
//   mt_ema      : t = β·t + (1-β)·s·scale_i  (model_average.py:87-131; scale_i = 1/σ_i
//                 absorbs spectral norm into the averaged model)
//   mt_scale    : x *= s (gradient clipping / unscale)
//   mt_sqnorm   : Σ x² per list (gradient-norm for clipping)
//   mt_fromage  : Fromage (optimizers/fromage.py): per-tensor |p|, |g| in a fixed-order reduce,
//                 then one update pass; the zero-norm branch is taken on the device
//   mt_madam    : Madam (optimizers/madam.py): per-parameter {step, max} live on the device
#include "common.h"

#include <cstdlib>
#include <type_traits>
#include <mutex>
#include <unordered_map>
#include <unordered_set>

namespace iamd {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 256 * 4 * 16;  // elements per workgroup (fp32: 64 KiB per operand)

struct TensorEntry {
  void* p[5];
  int64_t numel;
  int64_t cols;  // numel / size(0): row length when viewed as a matrix (spectral norm)
  // channels-last 4-D weights: memory column (kh, kw, ci) -> logical column (ci, kh, kw)
  int64_t cl_cin;  // 0 = memory order == logical order
  int64_t cl_khw;
};

struct Table {
  at::Tensor entries;  // device: TensorEntry[T]
  at::Tensor blocks;   // device: int2 {tensor, chunk} per workgroup
  int nblocks;
  const TensorEntry* ents() const {
    return reinterpret_cast<const TensorEntry*>(entries.data_ptr());
  }
  const int* blks() const { return blocks.data_ptr<int>(); }
};

std::mutex g_mu;
std::unordered_map<uint64_t, Table> g_cache;

}  // namespace

// ---- host -> device table staging that is safe under hipGraph capture -----------------------
// Outside a capture: pinned staging + async copy on the current stream (never blocks the
// host). During a capture no copy may be enqueued (a pageable/pinned H2D node would re-read a
// host buffer that is gone by replay time), so the device buffer is allocated (from the
// graph's private pool) and the upload is DEFERRED: flush_deferred_uploads() copies it
// synchronously after the capture has ended, before the first replay. Buffers created during
// a capture are also kept alive for the life of the process, so a later cache eviction can
// never free memory a graph still reads.
namespace {
struct Deferred {
  at::Tensor dst;
  std::vector<uint8_t> bytes;
};
std::mutex g_def_mu;
std::vector<Deferred> g_deferred;
std::vector<at::Tensor> g_graph_keep;
// Tables made during a capture are carved from a persistent arena allocated OUTSIDE any
// capture (regular caching-allocator memory): graph-pool memory allocated inside a capture
// belongs to the graph's own allocation nodes and need not hold host-written bytes at
// replay time.
constexpr int64_t kArenaBytes = 64ll << 20;
std::unordered_map<int, std::pair<at::Tensor, int64_t>> g_arena;

void ensure_arena(const at::Device& dev) {
  auto& a = g_arena[dev.index()];
  if (!a.first.defined())
    a = {at::empty({kArenaBytes}, at::TensorOptions().dtype(at::kByte).device(dev)), 0};
}
}  // namespace

bool stream_capturing() {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  IAMD_HIP_CHECK(hipStreamIsCapturing(stream(), &st));
  return st != hipStreamCaptureStatusNone;
}

at::Tensor stage_to_device(const void* src, size_t bytes, const at::Device& dev) {
  const int64_t n = (int64_t)std::max<size_t>(bytes, 1);
  if (stream_capturing()) {
    std::lock_guard<std::mutex> lk(g_def_mu);
    auto it = g_arena.find(dev.index());
    IAMD_CHECK(it != g_arena.end() && it->second.first.defined(),
               "no table arena: run the step once eagerly before capturing it");
    const int64_t off = (it->second.second + 255) / 256 * 256;
    IAMD_CHECK(off + n <= kArenaBytes, "capture table arena exhausted");
    auto d = it->second.first.narrow(0, off, n);
    it->second.second = off + n;
    Deferred df;
    df.dst = d;
    df.bytes.assign(reinterpret_cast<const uint8_t*>(src),
                    reinterpret_cast<const uint8_t*>(src) + bytes);
    g_deferred.push_back(std::move(df));
    g_graph_keep.push_back(d);
    return d;
  }
  {
    std::lock_guard<std::mutex> lk(g_def_mu);
    ensure_arena(dev);  // reserved at the first eager use, ready for a later capture
  }
  auto pin = at::TensorOptions().dtype(at::kByte).pinned_memory(true);
  auto h = at::empty({n}, pin);
  if (bytes) memcpy(h.data_ptr(), src, bytes);
  return h.to(dev, /*non_blocking=*/true);
}

void keep_for_graph(const at::Tensor& t) {
  if (!t.defined() || !stream_capturing()) return;
  static std::unordered_set<const void*> kept;
  std::lock_guard<std::mutex> lk(g_def_mu);
  const void* key = t.storage().unsafeGetStorageImpl();
  if (kept.insert(key).second) g_graph_keep.push_back(t);
}

int64_t flush_deferred_uploads() {
  std::lock_guard<std::mutex> lk(g_def_mu);
  const int64_t n = (int64_t)g_deferred.size();
  for (auto& d : g_deferred)
    if (!d.bytes.empty())
      IAMD_HIP_CHECK(hipMemcpy(d.dst.data_ptr(), d.bytes.data(), d.bytes.size(),
                               hipMemcpyHostToDevice));
  g_deferred.clear();
  return n;
}

namespace {

uint64_t mix(uint64_t h, uint64_t v) {
  h ^= v + 0x9e3779b97f4a7c15ULL + (h << 6) + (h >> 2);
  return h;
}

// Cache key of a tensor-list set. It covers everything an entry records: pointers, sizes and
// the memory layout (a freed tensor's address reused by one of another shape must not hit a
// stale entry). Every size and stride of list 0 is mixed on its own: folded into one sum, two
// channels-last weights of equal numel and size(0) met on one key with different
// (cl_cin, cl_khw).
uint64_t table_key(const std::vector<std::vector<at::Tensor>>& lists) {
  const size_t T = lists[0].size();
  uint64_t h = 1469598103934665603ULL ^ (uint64_t)lists.size();
  for (size_t i = 0; i < T; ++i) {
    for (auto& l : lists) {
      // (an empty tensor stands for "no operand": the optional bf16 shadow of a parameter)
      h = mix(h, l[i].numel() ? reinterpret_cast<uint64_t>(l[i].data_ptr()) : 0);
      h = mix(h, (uint64_t)l[i].numel());
    }
    const at::Tensor& t0 = lists[0][i];
    h = mix(h, (uint64_t)t0.dim());
    for (int64_t d = 0; d < t0.dim(); ++d) {
      h = mix(h, (uint64_t)t0.size(d));
      h = mix(h, (uint64_t)t0.stride(d));
    }
  }
  return h;
}

// Build (or fetch from cache) the device table for up to 5 parallel tensor lists.
Table& get_table(const std::vector<std::vector<at::Tensor>>& lists, const at::Device& dev) {
  const size_t T = lists[0].size();
  const uint64_t h = table_key(lists);
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_cache.find(h);
  if (it != g_cache.end()) {
    keep_for_graph(it->second.entries);
    keep_for_graph(it->second.blocks);
    return it->second;
  }
  std::vector<TensorEntry> ents(T);
  std::vector<int32_t> bm;
  for (size_t i = 0; i < T; ++i) {
    for (size_t k = 0; k < 5; ++k)
      ents[i].p[k] = (k < lists.size() && lists[k][i].numel()) ? lists[k][i].data_ptr() : nullptr;
    ents[i].numel = lists[0][i].numel();
    ents[i].cols = lists[0][i].dim() > 0 && lists[0][i].size(0) > 0
                       ? ents[i].numel / lists[0][i].size(0) : 1;
    const at::Tensor& t0 = lists[0][i];
    const bool cl = t0.dim() == 4 && !t0.is_contiguous() &&
                    t0.is_contiguous(at::MemoryFormat::ChannelsLast);
    ents[i].cl_cin = cl ? t0.size(1) : 0;
    ents[i].cl_khw = cl ? t0.size(2) * t0.size(3) : 0;
    // every parallel operand of the same rank must share the layout of list 0
    for (size_t k = 1; k < lists.size(); ++k)
      if (lists[k][i].dim() == t0.dim())
        IAMD_CHECK(lists[k][i].strides() == t0.strides(),
                   "multi-tensor: operand layouts differ (strides must match)");
    const int64_t nch = (ents[i].numel + kChunk - 1) / kChunk;
    for (int64_t c = 0; c < nch; ++c) {
      bm.push_back((int32_t)i);
      bm.push_back((int32_t)c);
    }
  }
  // pinned staging + async copy on the current stream (deferred under graph capture)
  Table t;
  t.entries = stage_to_device(ents.data(), T * sizeof(TensorEntry), dev);
  t.blocks = stage_to_device(bm.data(), bm.size() * sizeof(int32_t), dev).view(at::kInt);
  t.nblocks = (int)(bm.size() / 2);
  if (g_cache.size() > 256) g_cache.clear();
  auto res = g_cache.emplace(h, std::move(t));
  return res.first->second;
}

// Device-resident Adam hyper-parameters [lr, step, step_size, rsqrt(bc2)] (capturable
// optimizer step: the step count and the bias corrections live on the device, so a replayed
// hipGraph advances them instead of baking the capture-time values).
__global__ void adam_hyper_step(float* __restrict__ hyper, float beta1, float beta2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float step = hyper[1] + 1.f;
    hyper[1] = step;
    const float bc1 = 1.f - powf(beta1, step);
    const float bc2 = 1.f - powf(beta2, step);
    hyper[2] = hyper[0] / bc1;
    hyper[3] = rsqrtf(bc2);
  }
}

// Streaming (non-temporal) 16-B fp32 load / store: Adam touches every byte once per step, so
// its traffic need not displace L2 lines. 2.44 -> 2.39 ms for the 415M-parameter SPADE set
// (5.1 -> 5.2 TB/s, profiles/adam_nt_ab_r6_mi355x.txt); IMAGINAIRE_AMD_ADAM_NT=0 switches back.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ void ld4(const float* __restrict__ p, float (&o)[4]) {
  f32x4 v = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p))
               : *reinterpret_cast<const f32x4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <bool NT>
__device__ __forceinline__ void st4(float* __restrict__ p, const float (&i)[4]) {
  f32x4 v = {i[0], i[1], i[2], i[3]};
  if (NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
  else *reinterpret_cast<f32x4*>(p) = v;
}

// What a workgroup of the block map works on: its tensor's entry and the slice [start, end) of
// that tensor. start is a multiple of kChunk, so of every vector width used below.
struct Chunk {
  TensorEntry e;
  int t;
  int64_t start, end;
};
__device__ __forceinline__ Chunk block_chunk(const TensorEntry* __restrict__ ents,
                                             const int* __restrict__ blocks) {
  const int t = blocks[2 * blockIdx.x], chunk = blocks[2 * blockIdx.x + 1];
  const TensorEntry e = ents[t];
  const int64_t start = (int64_t)chunk * kChunk;
  return {e, t, start, min(e.numel, start + (int64_t)kChunk)};
}

// The loop of every streaming kernel over its chunk. vec_ok (every operand of the kernel on its
// vector alignment): groups of 4 elements per lane through load4(i, r) / apply4(i, r), then the
// last 1..3 elements through apply1(i); otherwise apply1 for every element. V holds one group's
// registers. U groups per lane per trip, all loads issued before any math: 4 x U 16-B loads in
// flight per lane and operand (one group at a time left Adam latency-bound at ~1.5 TB/s).
// kZeroFill: a group past the end is applied as zeros instead of skipped, so apply4 must not
// touch memory. For a pure reduction (fmaf(0, 0, acc) == acc) that keeps the accumulation one
// straight chain; branching round the groups cost fromage_norm_kernel 26 VGPRs and two waves of
// occupancy.
template <typename V, bool kZeroFill = false, typename Load4, typename Apply4, typename Apply1>
__device__ __forceinline__ void stream_chunk(const Chunk& c, bool vec_ok, Load4 load4,
                                             Apply4 apply4, Apply1 apply1) {
  if (vec_ok) {
    constexpr int U = 4;
    const int64_t vend = c.start + ((c.end - c.start) & ~(int64_t)3);
    for (int64_t base = c.start + threadIdx.x * 4; base < vend; base += kThreads * 4 * U) {
      V r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * kThreads * 4;
        if (i < vend) load4(i, r[u]);
        else if (kZeroFill) r[u] = V{};
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * kThreads * 4;
        if (kZeroFill || i < vend) apply4(i, r[u]);
      }
    }
    for (int64_t i = vend + threadIdx.x; i < c.end; i += kThreads) apply1(i);
  } else {
    for (int64_t i = c.start + threadIdx.x; i < c.end; i += kThreads) apply1(i);
  }
}

template <typename G, bool NT>
__global__ void __launch_bounds__(kThreads)
adam_kernel(const TensorEntry* __restrict__ ents, const int* __restrict__ blocks, float lr,
            float beta1, float beta2, float eps, float bc1, float bc2, float wd, int adamw,
            float grad_scale, const float* __restrict__ hyper) {
  const Chunk c = block_chunk(ents, blocks);
  float* __restrict__ p = reinterpret_cast<float*>(c.e.p[0]);
  const G* __restrict__ g = reinterpret_cast<const G*>(c.e.p[1]);
  float* __restrict__ m = reinterpret_cast<float*>(c.e.p[2]);
  float* __restrict__ v = reinterpret_cast<float*>(c.e.p[3]);
  __hip_bfloat16* __restrict__ shadow = reinterpret_cast<__hip_bfloat16*>(c.e.p[4]);
  float step_size, rbc2;
  if (hyper) {
    lr = hyper[0];
    step_size = hyper[2];
    rbc2 = hyper[3];
  } else {
    step_size = lr / bc1;
    rbc2 = rsqrtf(bc2);
  }
  struct V { float p[4], g[4], m[4], v[4]; };
  auto update = [&](float& pv, float gv, float& mv, float& vv) {
    float gr = gv * grad_scale;
    if (!adamw && wd != 0.f) gr = fmaf(wd, pv, gr);
    mv = fmaf(beta1, mv, (1.f - beta1) * gr);
    vv = fmaf(beta2, vv, (1.f - beta2) * gr * gr);
    const float denom = sqrtf(vv) * rbc2 + eps;
    if (adamw && wd != 0.f) pv *= (1.f - lr * wd);
    pv -= step_size * mv / denom;
  };
  // (the shadow, when there is one, is written 4 bf16 = 8 bytes at a time; null passes)
  const bool vec_ok = (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) % 16 == 0) &&
                      ((uintptr_t)g % (4 * sizeof(G)) == 0) && ((uintptr_t)shadow % 8 == 0);
  stream_chunk<V>(
      c, vec_ok,
      [&](int64_t i, V& r) {
        ld4<NT>(p + i, r.p);
        load_vec<G, 4>(g + i, r.g);
        ld4<NT>(m + i, r.m);
        ld4<NT>(v + i, r.v);
      },
      [&](int64_t i, V& r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) update(r.p[k], r.g[k], r.m[k], r.v[k]);
        st4<NT>(p + i, r.p);
        st4<NT>(m + i, r.m);
        st4<NT>(v + i, r.v);
        if (shadow) store_vec<__hip_bfloat16, 4>(shadow + i, r.p);
      },
      [&](int64_t i) {
        float pv = p[i], mv = m[i], vv = v[i];
        update(pv, to_f<G>(g[i]), mv, vv);
        p[i] = pv; m[i] = mv; v[i] = vv;
        if (shadow) shadow[i] = __float2bfloat16(pv);
      });
}

// σ_i = Σ_{r,c} u[r] W[r,c] v[c]  (W viewed as [rows, numel/rows]); one partial per chunk.
// entry: p0 = W (fp32), p1 = u, p2 = v; rows carried in the sigma-rows array.
__global__ void __launch_bounds__(kThreads)
sn_sigma_kernel(const TensorEntry* __restrict__ ents, const int* __restrict__ blocks,
                float* __restrict__ part) {
  __shared__ float sh[kThreads / 64];
  const Chunk ch = block_chunk(ents, blocks);
  const float* __restrict__ W = reinterpret_cast<const float*>(ch.e.p[0]);
  const float* __restrict__ u = reinterpret_cast<const float*>(ch.e.p[1]);
  // p[3]: v permuted to the weight's MEMORY column order by sn_vperm (coalesced reads; the
  // logical-order v of a channels-last conv weight would be a stride-KH*KW gather)
  const float* __restrict__ v = reinterpret_cast<const float*>(ch.e.p[3]);
  const int64_t ncol = ch.e.cols;
  const int64_t start = ch.start, end = ch.end;
  float acc = 0.f;
  if ((ncol & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0 &&
      (reinterpret_cast<uintptr_t>(v) & 15) == 0) {
    // 4 consecutive elements (one row: ncol % 4 == 0) per lane and trip, 16-B loads of W and v;
    // chunk starts are multiples of 4 (kChunk % 4 == 0)
    const int64_t i0 = start + threadIdx.x * 4;
    int64_t r = i0 / ncol;
    int64_t c = i0 - r * ncol;
    for (int64_t i = i0; i < end; i += kThreads * 4) {
      const float4 w4 = *reinterpret_cast<const float4*>(W + i);
      const float4 v4 = *reinterpret_cast<const float4*>(v + c);
      acc = fmaf(u[r], fmaf(w4.x, v4.x, fmaf(w4.y, v4.y, fmaf(w4.z, v4.z, w4.w * v4.w))), acc);
      c += kThreads * 4;
      while (c >= ncol) { c -= ncol; ++r; }
    }
  } else {
    // (row, column) walked incrementally: no 64-bit division per element
    const int64_t i0 = start + threadIdx.x;
    int64_t r = i0 / ncol;
    int64_t c = i0 - r * ncol;
    for (int64_t i = i0; i < end; i += kThreads) {
      acc = fmaf(u[r] * W[i], v[c], acc);
      c += kThreads;
      while (c >= ncol) { c -= ncol; ++r; }
    }
  }
  // per-workgroup partial; reduce_block_partials sums them in a fixed order
  const float s = block_sum<kThreads>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out[t][n] = Σ_{b : blocks[b].tensor == t} part[b][n] for the N values per workgroup, one
// workgroup per tensor (T = 1 with all_blocks: every partial). Fixed per-thread strides + a
// fixed tree: bitwise reproducible, unlike one float atomic per workgroup (whose arrival order
// varies run to run).
template <int N>
__global__ void __launch_bounds__(kThreads)
reduce_block_partials(const float* __restrict__ part, const int* __restrict__ blocks, int nblocks,
                      bool all_blocks, float* __restrict__ out) {
  __shared__ float sh[N * (kThreads / 64)];
  const int t = blockIdx.x;
  float acc[N];
#pragma unroll
  for (int n = 0; n < N; ++n) acc[n] = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += kThreads)
    if (all_blocks || blocks[2 * b] == t) {
#pragma unroll
      for (int n = 0; n < N; ++n) acc[n] += part[N * b + n];
    }
  const float s = block_sum<kThreads, N>(acc, sh);
  if (threadIdx.x < N) out[N * t + threadIdx.x] = s;
}

// one block per tensor: vm[c] = v[logical(c)] for every memory column c
__global__ void __launch_bounds__(kThreads)
sn_vperm(const TensorEntry* __restrict__ ents) {
  const TensorEntry e = ents[blockIdx.x];
  const float* __restrict__ v = reinterpret_cast<const float*>(e.p[2]);
  float* __restrict__ vm = reinterpret_cast<float*>(e.p[3]);
  const uint32_t cin = (uint32_t)e.cl_cin;
  for (int64_t c = threadIdx.x; c < e.cols; c += kThreads) {
    int64_t lc = c;
    if (cin) {
      const uint32_t q = (uint32_t)c / cin;
      lc = (int64_t)((uint32_t)c - q * cin) * e.cl_khw + q;
    }
    vm[c] = v[lc];
  }
}

// t = beta*t + (1-beta)*s*scale[t_idx]; p0 = target, p1 = source (same dtype).
// The 16-B path is for fp32 only. NT: the average itself is streamed (non-temporal fp32 load /
// store: nothing else in the step reads it): 0.962 -> 0.928 ms for 415M parameters
// (profiles/ema_nt_ab_r6_mi355x.txt); IMAGINAIRE_AMD_EMA_NT=0 switches back to plain accesses.
template <typename T, bool NT>
__global__ void __launch_bounds__(kThreads)
ema_kernel(const TensorEntry* __restrict__ ents, const int* __restrict__ blocks, float beta,
           const float* __restrict__ inv_scale, const int64_t* __restrict__ count,
           int64_t warm_until) {
  const Chunk c = block_chunk(ents, blocks);
  // device-side warm-up switch (model_average.py: beta = 0 until start_iteration), so a
  // replayed hipGraph turns the average on at the right iteration
  if (count && *count <= warm_until) beta = 0.f;
  T* __restrict__ dst = reinterpret_cast<T*>(c.e.p[0]);
  const T* __restrict__ src = reinterpret_cast<const T*>(c.e.p[1]);
  const float sc = inv_scale ? 1.f / inv_scale[c.t] : 1.f;
  const float a = 1.f - beta;
  const float as = a * sc;
  struct V { float d[4], s[4]; };
  auto update = [&](float dv, float sv) { return fmaf(beta, dv, as * sv); };
  const bool vec_ok = sizeof(T) == 4 && (((uintptr_t)dst | (uintptr_t)src) & 15) == 0;
  stream_chunk<V>(
      c, vec_ok,
      [&](int64_t i, V& r) {
        if constexpr (std::is_same<T, float>::value) ld4<NT>(dst + i, r.d);
        else load_vec<T, 4>(dst + i, r.d);
        load_vec<T, 4>(src + i, r.s);
      },
      [&](int64_t i, V& r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.d[k] = update(r.d[k], r.s[k]);
        if constexpr (std::is_same<T, float>::value) st4<NT>(dst + i, r.d);
        else store_vec<T, 4>(dst + i, r.d);
      },
      [&](int64_t i) { dst[i] = from_f<T>(update(to_f<T>(dst[i]), to_f<T>(src[i]))); });
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
scale_kernel(const TensorEntry* __restrict__ ents, const int* __restrict__ blocks,
             const float* __restrict__ s) {
  const Chunk c = block_chunk(ents, blocks);
  T* __restrict__ x = reinterpret_cast<T*>(c.e.p[0]);
  const float f = *s;
  for (int64_t i = c.start + threadIdx.x; i < c.end; i += kThreads)
    x[i] = from_f<T>(to_f<T>(x[i]) * f);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
sqnorm_kernel(const TensorEntry* __restrict__ ents, const int* __restrict__ blocks,
              float* __restrict__ part) {
  __shared__ float sh[kThreads / 64];
  const Chunk c = block_chunk(ents, blocks);
  const T* __restrict__ x = reinterpret_cast<const T*>(c.e.p[0]);
  float acc = 0.f;
  for (int64_t i = c.start + threadIdx.x; i < c.end; i += kThreads) {
    const float v = to_f<T>(x[i]);
    acc = fmaf(v, v, acc);
  }
  const float s = block_sum<kThreads>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- Fromage / Madam (reference optimizers/fromage.py, optimizers/madam.py) --------------------
// Everything a step decides (Fromage's zero-norm branch, Madam's bias correction and clamp bound)
// is decided on the device, so the step records into a hipGraph as it is. Their fp32 operands
// are always streamed (non-temporal).

// Fromage pass 1: part[b] = {Σ p², Σ g²} over workgroup b's chunk. p0 = p (fp32), p1 = g.
template <typename G>
__global__ void __launch_bounds__(kThreads)
fromage_norm_kernel(const TensorEntry* __restrict__ ents, const int* __restrict__ blocks,
                    float* __restrict__ part) {
  __shared__ float sh[2 * (kThreads / 64)];
  const Chunk c = block_chunk(ents, blocks);
  const float* __restrict__ p = reinterpret_cast<const float*>(c.e.p[0]);
  const G* __restrict__ g = reinterpret_cast<const G*>(c.e.p[1]);
  float acc[2] = {0.f, 0.f};  // {Σ p², Σ g²} of this lane
  struct V { float p[4], g[4]; };
  auto update = [&](float pv, float gv) {
    acc[0] = fmaf(pv, pv, acc[0]);
    acc[1] = fmaf(gv, gv, acc[1]);
  };
  const bool vec_ok = ((uintptr_t)p % 16 == 0) && ((uintptr_t)g % (4 * sizeof(G)) == 0);
  stream_chunk<V, /*kZeroFill=*/true>(
      c, vec_ok,
      [&](int64_t i, V& r) {
        ld4<true>(p + i, r.p);
        load_vec<G, 4>(g + i, r.g);
      },
      [&](int64_t, V& r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) update(r.p[k], r.g[k]);
      },
      [&](int64_t i) { update(p[i], to_f<G>(g[i])); });
  const float s = block_sum<kThreads, 2>(acc, sh);
  if (threadIdx.x < 2) part[2 * blockIdx.x + threadIdx.x] = s;
}

// Fromage pass 2: p = (p - lr * ratio * g) / sqrt(1 + lr²), ratio = |p| / |g| of the whole
// tensor when both norms are positive, else 1 (taken per tensor, here). p2 = bf16 shadow.
template <typename G>
__global__ void __launch_bounds__(kThreads)
fromage_kernel(const TensorEntry* __restrict__ ents, const int* __restrict__ blocks,
               const float* __restrict__ norms, float lr, const float* __restrict__ hyper) {
  const Chunk ch = block_chunk(ents, blocks);
  float* __restrict__ p = reinterpret_cast<float*>(ch.e.p[0]);
  const G* __restrict__ g = reinterpret_cast<const G*>(ch.e.p[1]);
  __hip_bfloat16* __restrict__ shadow = reinterpret_cast<__hip_bfloat16*>(ch.e.p[2]);
  if (hyper) lr = hyper[0];
  const float pn = sqrtf(norms[2 * ch.t]), gn = sqrtf(norms[2 * ch.t + 1]);
  const float na = -lr * ((pn > 0.f && gn > 0.f) ? pn / gn : 1.f);
  const float c = 1.f / sqrtf(fmaf(lr, lr, 1.f));
  struct V { float p[4], g[4]; };
  auto update = [&](float pv, float gv) { return fmaf(na, gv, pv) * c; };
  const bool vec_ok = ((uintptr_t)p % 16 == 0) && ((uintptr_t)g % (4 * sizeof(G)) == 0) &&
                      ((uintptr_t)shadow % 8 == 0);
  stream_chunk<V>(
      ch, vec_ok,
      [&](int64_t i, V& r) {
        ld4<true>(p + i, r.p);
        load_vec<G, 4>(g + i, r.g);
      },
      [&](int64_t i, V& r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.p[k] = update(r.p[k], r.g[k]);
        st4<true>(p + i, r.p);
        if (shadow) store_vec<__hip_bfloat16, 4>(shadow + i, r.p);
      },
      [&](int64_t i) {
        const float pv = update(p[i], to_f<G>(g[i]));
        p[i] = pv;
        if (shadow) shadow[i] = __float2bfloat16(pv);
      });
}

// Madam's per-parameter device state is {step, max} (fp32): slot p1 of mt_madam_init's table,
// slot p4 of mt_madam's. Here: state[1] = scale * sqrt(mean(p²)) from the per-tensor Σ p².
__global__ void __launch_bounds__(kThreads)
madam_max_kernel(const TensorEntry* __restrict__ ents, int ntensors,
                 const float* __restrict__ sums, float scale) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= ntensors) return;
  float* __restrict__ st = reinterpret_cast<float*>(ents[t].p[1]);
  const int64_t n = ents[t].numel;
  if (st) st[1] = n > 0 ? scale * sqrtf(sums[t] / (float)n) : 0.f;
}

// Prologue of every Madam step: each listed parameter's own step count moves on by one.
__global__ void __launch_bounds__(kThreads)
madam_step_kernel(const TensorEntry* __restrict__ ents, int ntensors) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= ntensors) return;
  float* __restrict__ st = reinterpret_cast<float*>(ents[t].p[4]);
  if (st) st[0] += 1.f;
}

// One Madam update of an element. sbc = sqrt(bias correction): g / sqrt(v / bc) is evaluated as
// g * sqrt(bc) / sqrt(v), one square root and one division per element.
__device__ __forceinline__ void madam_update(float& p, float g, float& v, float sbc, float nlr,
                                             float bound, float mx) {
  v = fmaf(0.999f, v, 0.001f * (g * g));
  float gn = g * sbc / sqrtf(v);
  gn = gn != gn ? 0.f : gn;  // 0 / 0: a gradient that has been zero since the first step
  if (bound >= 0.f) gn = fminf(fmaxf(gn, -bound), bound);
  const float sg = p > 0.f ? 1.f : (p < 0.f ? -1.f : 0.f);
  p *= expf(nlr * gn * sg);
  p = fminf(fmaxf(p, -mx), mx);
}

// p0 = p (fp32), p1 = g, p2 = exp_avg_sq, p3 = bf16 shadow, p4 = state {step, max}.
// bound < 0: no gradient clamp.
template <typename G>
__global__ void __launch_bounds__(kThreads)
madam_kernel(const TensorEntry* __restrict__ ents, const int* __restrict__ blocks, float lr,
             float bound, const float* __restrict__ hyper) {
  const Chunk c = block_chunk(ents, blocks);
  float* __restrict__ p = reinterpret_cast<float*>(c.e.p[0]);
  const G* __restrict__ g = reinterpret_cast<const G*>(c.e.p[1]);
  float* __restrict__ v = reinterpret_cast<float*>(c.e.p[2]);
  __hip_bfloat16* __restrict__ shadow = reinterpret_cast<__hip_bfloat16*>(c.e.p[3]);
  const float* __restrict__ st = reinterpret_cast<const float*>(c.e.p[4]);
  if (hyper) lr = hyper[0];
  const float nlr = -lr;
  // once per workgroup: bc = 1 - 0.999^step = -expm1(step * ln 0.999) (the form that keeps its
  // precision at small step counts, where 0.999^step is close to 1)
  const float sbc = sqrtf(-expm1f(st[0] * -1.0005003335835335e-3f));
  const float mx = st[1];
  struct V { float p[4], g[4], v[4]; };
  const bool vec_ok = (((uintptr_t)p | (uintptr_t)v) % 16 == 0) &&
                      ((uintptr_t)g % (4 * sizeof(G)) == 0) && ((uintptr_t)shadow % 8 == 0);
  stream_chunk<V>(
      c, vec_ok,
      [&](int64_t i, V& r) {
        ld4<true>(p + i, r.p);
        load_vec<G, 4>(g + i, r.g);
        ld4<true>(v + i, r.v);
      },
      [&](int64_t i, V& r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) madam_update(r.p[k], r.g[k], r.v[k], sbc, nlr, bound, mx);
        st4<true>(v + i, r.v);
        st4<true>(p + i, r.p);
        if (shadow) store_vec<__hip_bfloat16, 4>(shadow + i, r.p);
      },
      [&](int64_t i) {
        float pv = p[i], vv = v[i];
        madam_update(pv, to_f<G>(g[i]), vv, sbc, nlr, bound, mx);
        v[i] = vv; p[i] = pv;
        if (shadow) shadow[i] = __float2bfloat16(pv);
      });
}

void check_same_dtype(const std::vector<at::Tensor>& l, at::ScalarType st, const char* what) {
  for (auto& t : l) {
    IAMD_CHECK(t.scalar_type() == st, what, ": dtype mismatch");
    IAMD_CHECK(t.is_non_overlapping_and_dense(), what, ": tensors must be dense");
  }
}

// The device hyper-parameters of an optimizer step, learning rate first: a replayed graph sees
// a changed value. Null = none given, use the host arguments.
float* lr_hyper(const c10::optional<at::Tensor>& hyper, const char* what, int64_t min_numel = 1) {
  if (!hyper.has_value() || !hyper->defined()) return nullptr;
  IAMD_CHECK(hyper->is_cuda() && hyper->scalar_type() == at::kFloat &&
                 hyper->numel() >= min_numel && hyper->is_contiguous(),
             what, ": hyper must be a contiguous fp32 device tensor [lr, ...] of at least ",
             min_numel, " floats");
  return hyper->data_ptr<float>();
}

// Optional bf16 shadows, one per parameter (an empty tensor = none for that parameter); an empty
// list = none at all, returned as a list of empty tensors so the table slots stay put.
std::vector<at::Tensor> shadow_list(const std::vector<at::Tensor>& shadows,
                                    const std::vector<at::Tensor>& params, const char* what) {
  if (shadows.empty())
    return std::vector<at::Tensor>(params.size(),
                                   at::empty({0}, params[0].options().dtype(at::kBFloat16)));
  IAMD_CHECK(shadows.size() == params.size(), what, ": shadow list size");
  for (size_t i = 0; i < shadows.size(); ++i) {
    if (shadows[i].numel() == 0) continue;
    IAMD_CHECK(shadows[i].scalar_type() == at::kBFloat16 && shadows[i].is_cuda() &&
                   shadows[i].sizes() == params[i].sizes() &&
                   shadows[i].strides() == params[i].strides(),
               what, ": a shadow must be a bf16 tensor laid out like its parameter");
  }
  return shadows;
}

// fn(tag) with a null pointer of the gradients' element type
template <typename F>
void dispatch_grad(at::ScalarType gdt, const char* name, F fn) {
  if (gdt == at::kFloat) fn(static_cast<float*>(nullptr));
  else if (gdt == at::kBFloat16) fn(static_cast<__hip_bfloat16*>(nullptr));
  else IAMD_CHECK(false, name, ": grads must be fp32 or bf16");
}

// A switch that is on unless the environment variable starts with 0.
bool env_default_on(const char* name) {
  const char* e = std::getenv(name);
  return !(e && e[0] == '0');
}

}  // namespace

// Read-only view of the table cache key for tests: builds, caches and launches nothing.
uint64_t mt_table_key(const std::vector<std::vector<at::Tensor>>& lists) {
  IAMD_CHECK(!lists.empty() && lists.size() <= 5, "mt_table_key: 1 to 5 lists");
  for (auto& l : lists)
    IAMD_CHECK(l.size() == lists[0].size(), "mt_table_key: list sizes differ");
  return table_key(lists);
}

void mt_adam(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
             const std::vector<at::Tensor>& exp_avgs, const std::vector<at::Tensor>& exp_avg_sqs,
             const std::vector<at::Tensor>& shadows, double lr, double beta1, double beta2,
             double eps, int64_t step, double weight_decay, bool adamw, double grad_scale,
             const c10::optional<at::Tensor>& hyper) {
  if (params.empty()) return;
  float* hp = lr_hyper(hyper, "mt_adam", 4);  // [lr, step, step_size, rsqrt(bc2)]
  IAMD_CHECK(params.size() == grads.size() && params.size() == exp_avgs.size() &&
                 params.size() == exp_avg_sqs.size(),
             "mt_adam: list sizes differ");
  check_same_dtype(params, at::kFloat, "mt_adam params");
  check_same_dtype(exp_avgs, at::kFloat, "mt_adam exp_avg");
  check_same_dtype(exp_avg_sqs, at::kFloat, "mt_adam exp_avg_sq");
  const auto gdt = grads[0].scalar_type();
  check_same_dtype(grads, gdt, "mt_adam grads");
  Table& tb = get_table({params, grads, exp_avgs, exp_avg_sqs,
                         shadow_list(shadows, params, "mt_adam")}, params[0].device());
  const float bc1 = 1.f - (float)std::pow(beta1, (double)step);
  const float bc2 = 1.f - (float)std::pow(beta2, (double)step);
  if (hp)
    hipLaunchKernelGGL(adam_hyper_step, dim3(1), dim3(64), 0, stream(), hp, (float)beta1,
                       (float)beta2);
  static const bool nt = env_default_on("IMAGINAIRE_AMD_ADAM_NT");
  dispatch_grad(gdt, "mt_adam", [&](auto tag) {
    using G = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL((nt ? adam_kernel<G, true> : adam_kernel<G, false>), dim3(tb.nblocks),
                       dim3(kThreads), 0, stream(), tb.ents(), tb.blks(), (float)lr, (float)beta1,
                       (float)beta2, (float)eps, bc1, bc2, (float)weight_decay, adamw ? 1 : 0,
                       (float)grad_scale, hp);
  });
  IAMD_LAUNCH_CHECK();
}

at::Tensor mt_sn_sigma(const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& us,
                       const std::vector<at::Tensor>& vs) {
  IAMD_CHECK(!weights.empty(), "mt_sn_sigma: empty list");
  check_same_dtype(weights, at::kFloat, "mt_sn_sigma W");
  check_same_dtype(us, at::kFloat, "mt_sn_sigma u");
  check_same_dtype(vs, at::kFloat, "mt_sn_sigma v");
  // persistent per-device workspace for the memory-order v copies: stable pointers keep the
  // cached device table valid across calls
  static std::mutex ws_mu;
  static std::unordered_map<int, at::Tensor> ws_map;
  int64_t total = 0;
  for (auto& w : weights) total += w.numel() / std::max<int64_t>(1, w.size(0));
  std::vector<at::Tensor> vms;
  {
    std::lock_guard<std::mutex> lk(ws_mu);
    const int dev = weights[0].get_device();
    at::Tensor& ws = ws_map[dev];
    if (!ws.defined() || ws.numel() < total) {
      // an old workspace that a captured graph names is never freed (kept by keep_for_graph);
      // one only ever used eagerly is released with its last reference
      ws = at::empty({total}, weights[0].options());
    }
    keep_for_graph(ws);  // (no-op outside a capture)
    int64_t off = 0;
    for (auto& w : weights) {
      const int64_t cols = w.numel() / std::max<int64_t>(1, w.size(0));
      vms.push_back(ws.narrow(0, off, cols));
      off += cols;
    }
  }
  Table& tb = get_table({weights, us, vs, vms}, weights[0].device());
  auto sigma = at::empty({(int64_t)weights.size()}, weights[0].options());
  auto part = at::empty({(int64_t)tb.nblocks}, weights[0].options());
  hipLaunchKernelGGL(sn_vperm, dim3((unsigned)weights.size()), dim3(kThreads), 0, stream(),
                     tb.ents());
  hipLaunchKernelGGL(sn_sigma_kernel, dim3(tb.nblocks), dim3(kThreads), 0, stream(), tb.ents(),
                     tb.blks(), part.data_ptr<float>());
  hipLaunchKernelGGL(reduce_block_partials<1>, dim3((unsigned)weights.size()), dim3(kThreads), 0,
                     stream(), part.data_ptr<float>(), tb.blks(), tb.nblocks, false,
                     sigma.data_ptr<float>());
  IAMD_LAUNCH_CHECK();
  return sigma;
}

void mt_ema(const std::vector<at::Tensor>& targets, const std::vector<at::Tensor>& sources,
            double beta, const c10::optional<at::Tensor>& sigma,
            const c10::optional<at::Tensor>& count, int64_t start) {
  if (targets.empty()) return;
  const int64_t* cp = nullptr;
  if (count.has_value() && count->defined()) {
    IAMD_CHECK(count->is_cuda() && count->scalar_type() == at::kLong && count->numel() == 1,
               "mt_ema: count must be a 1-element int64 device tensor");
    cp = count->data_ptr<int64_t>();
  }
  const auto dt = targets[0].scalar_type();
  check_same_dtype(targets, dt, "mt_ema targets");
  check_same_dtype(sources, dt, "mt_ema sources");
  Table& tb = get_table({targets, sources}, targets[0].device());
  const float* sp = nullptr;
  if (sigma.has_value() && sigma->defined()) {
    IAMD_CHECK(sigma->numel() == (int64_t)targets.size() && sigma->scalar_type() == at::kFloat,
               "mt_ema: sigma must be fp32 [T]");
    sp = sigma->data_ptr<float>();
  }
  static const bool nt = env_default_on("IMAGINAIRE_AMD_EMA_NT");
  IAMD_DISPATCH_FLOAT_TYPES(dt, "mt_ema", [&] {
    hipLaunchKernelGGL((nt ? ema_kernel<scalar_t, true> : ema_kernel<scalar_t, false>),
                       dim3(tb.nblocks), dim3(kThreads), 0, stream(), tb.ents(), tb.blks(),
                       (float)beta, sp, cp, start);
  });
  IAMD_LAUNCH_CHECK();
}

void mt_scale(const std::vector<at::Tensor>& xs, const at::Tensor& s) {
  if (xs.empty()) return;
  const auto dt = xs[0].scalar_type();
  check_same_dtype(xs, dt, "mt_scale");
  Table& tb = get_table({xs}, xs[0].device());
  auto sf = s.to(at::kFloat).contiguous();
  IAMD_DISPATCH_FLOAT_TYPES(dt, "mt_scale", [&] {
    hipLaunchKernelGGL((scale_kernel<scalar_t>), dim3(tb.nblocks), dim3(kThreads), 0, stream(),
                       tb.ents(), tb.blks(), sf.data_ptr<float>());
  });
  IAMD_LAUNCH_CHECK();
}

at::Tensor mt_sqnorm(const std::vector<at::Tensor>& xs) {
  IAMD_CHECK(!xs.empty(), "mt_sqnorm: empty");
  const auto dt = xs[0].scalar_type();
  check_same_dtype(xs, dt, "mt_sqnorm");
  Table& tb = get_table({xs}, xs[0].device());
  auto out = at::empty({1}, xs[0].options().dtype(at::kFloat));
  auto part = at::empty({(int64_t)tb.nblocks}, xs[0].options().dtype(at::kFloat));
  IAMD_DISPATCH_FLOAT_TYPES(dt, "mt_sqnorm", [&] {
    hipLaunchKernelGGL((sqnorm_kernel<scalar_t>), dim3(tb.nblocks), dim3(kThreads), 0, stream(),
                       tb.ents(), tb.blks(), part.data_ptr<float>());
  });
  hipLaunchKernelGGL(reduce_block_partials<1>, dim3(1), dim3(kThreads), 0, stream(),
                     part.data_ptr<float>(), tb.blks(), tb.nblocks, true, out.data_ptr<float>());
  IAMD_LAUNCH_CHECK();
  return out;
}

namespace {

void check_madam_states(const std::vector<at::Tensor>& states, size_t n, const char* what) {
  IAMD_CHECK(states.size() == n, what, ": state list size");
  for (auto& s : states)
    IAMD_CHECK(s.is_cuda() && s.scalar_type() == at::kFloat && s.dim() == 1 && s.numel() == 2 &&
                   s.is_contiguous(),
               what, ": a state must be a contiguous fp32 device tensor [step, max]");
}

}  // namespace

void mt_fromage(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                const std::vector<at::Tensor>& shadows, double lr,
                const c10::optional<at::Tensor>& hyper) {
  if (params.empty()) return;
  const float* hp = lr_hyper(hyper, "mt_fromage");
  IAMD_CHECK(params.size() == grads.size(), "mt_fromage: list sizes differ");
  check_same_dtype(params, at::kFloat, "mt_fromage params");
  const auto gdt = grads[0].scalar_type();
  check_same_dtype(grads, gdt, "mt_fromage grads");
  dispatch_grad(gdt, "mt_fromage", [&](auto tag) {
    using G = std::remove_pointer_t<decltype(tag)>;
    Table& tb = get_table({params, grads, shadow_list(shadows, params, "mt_fromage")},
                          params[0].device());
    if (tb.nblocks == 0) return;
    const int T = (int)params.size();
    // (both fully written by the kernels below: no memset node in a captured step)
    auto part = at::empty({(int64_t)tb.nblocks, 2}, params[0].options());
    auto norms = at::empty({(int64_t)T, 2}, params[0].options());
    hipLaunchKernelGGL((fromage_norm_kernel<G>), dim3(tb.nblocks), dim3(kThreads), 0, stream(),
                       tb.ents(), tb.blks(), part.data_ptr<float>());
    hipLaunchKernelGGL(reduce_block_partials<2>, dim3(T), dim3(kThreads), 0, stream(),
                       part.data_ptr<float>(), tb.blks(), tb.nblocks, false,
                       norms.data_ptr<float>());
    hipLaunchKernelGGL((fromage_kernel<G>), dim3(tb.nblocks), dim3(kThreads), 0, stream(),
                       tb.ents(), tb.blks(), norms.data_ptr<float>(), (float)lr, hp);
  });
  IAMD_LAUNCH_CHECK();
}

// state[i][1] = scale * sqrt(mean(params[i]²)): Madam's clamp bound, taken from a parameter
// before its first update, without a host read.
void mt_madam_init(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& states,
                   double scale) {
  if (params.empty()) return;
  check_same_dtype(params, at::kFloat, "mt_madam_init params");
  check_madam_states(states, params.size(), "mt_madam_init");
  Table& tb = get_table({params, states}, params[0].device());
  const int T = (int)params.size();
  auto sums = at::empty({(int64_t)T}, params[0].options());
  auto part = at::empty({(int64_t)std::max(tb.nblocks, 1)}, params[0].options());
  if (tb.nblocks)
    hipLaunchKernelGGL((sqnorm_kernel<float>), dim3(tb.nblocks), dim3(kThreads), 0, stream(),
                       tb.ents(), tb.blks(), part.data_ptr<float>());
  hipLaunchKernelGGL(reduce_block_partials<1>, dim3(T), dim3(kThreads), 0, stream(),
                     part.data_ptr<float>(), tb.blks(), tb.nblocks, false,
                     sums.data_ptr<float>());
  hipLaunchKernelGGL(madam_max_kernel, dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream(), tb.ents(), T, sums.data_ptr<float>(), (float)scale);
  IAMD_LAUNCH_CHECK();
}

void mt_madam(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
              const std::vector<at::Tensor>& exp_avg_sqs, const std::vector<at::Tensor>& shadows,
              const std::vector<at::Tensor>& states, double lr,
              const c10::optional<double>& g_bound, const c10::optional<at::Tensor>& hyper) {
  if (params.empty()) return;
  const float* hp = lr_hyper(hyper, "mt_madam");
  IAMD_CHECK(params.size() == grads.size() && params.size() == exp_avg_sqs.size(),
             "mt_madam: list sizes differ");
  check_same_dtype(params, at::kFloat, "mt_madam params");
  check_same_dtype(exp_avg_sqs, at::kFloat, "mt_madam exp_avg_sq");
  const auto gdt = grads[0].scalar_type();
  check_same_dtype(grads, gdt, "mt_madam grads");
  check_madam_states(states, params.size(), "mt_madam");
  IAMD_CHECK(!g_bound.has_value() || *g_bound >= 0.0, "mt_madam: g_bound must be >= 0 or None");
  const float bound = g_bound.has_value() ? (float)*g_bound : -1.f;
  dispatch_grad(gdt, "mt_madam", [&](auto tag) {
    using G = std::remove_pointer_t<decltype(tag)>;
    Table& tb = get_table({params, grads, exp_avg_sqs, shadow_list(shadows, params, "mt_madam"),
                           states}, params[0].device());
    const int T = (int)params.size();
    hipLaunchKernelGGL(madam_step_kernel, dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       stream(), tb.ents(), T);
    if (tb.nblocks)
      hipLaunchKernelGGL((madam_kernel<G>), dim3(tb.nblocks), dim3(kThreads), 0, stream(),
                         tb.ents(), tb.blks(), (float)lr, bound, hp);
  });
  IAMD_LAUNCH_CHECK();
}

}  // namespace iamd
