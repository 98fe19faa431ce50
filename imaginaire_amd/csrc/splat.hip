// k18: device-side point-cloud splat renderer (world-consistent vid2vid guidance).
//
// Replaces the host path of reference model_utils/wc_vid2vid/render.py:63-147 (numpy colour /
// seen / first-seen-time arrays that grow with the largest point id, updated and rendered with
// fancy-index assignments) with a cloud of FIXED capacity P that lives on the device and is
// only ever modified in place, so a hipGraph keeps valid pointers and every replay follows the
// batch's own rows and counts (both read on the device).
//
// State per sample b: color[b, P] (one word per point: R | G << 8 | B << 16 | seen << 24),
// seen_time[b, P], counters[b, 4] = (call_idx, dropped rows, 0, 0), and two "winner" tables,
// win_pt[b, P] and win_px[b, h * w], that hold -1 between calls.
//
// Duplicate targets resolve as numpy's fancy assignment does: the LAST row wins. Both
// operations run two passes:
//   1. every valid row does an integer atomicMax of its row number into its target's winner
//      word (point id for the update, pixel for the render);
//   2. update: the row that equals its point's winner resets that word to -1 and, if the point
//      is unseen, stores the quantised pixel and call_idx (a losing row that reads the -1 of an
//      already reset word loses as well); render: one thread per pixel group reads the winner,
//      resets it to -1 and writes all four output channels, background where no row won.
// So nothing is zeroed per call (no memset node), no float atomics run, the result does not
// depend on the order in which blocks execute, and every output element is written.
//
// Rows that cannot be applied (point id outside [0, P), pixel outside the image) never address
// memory: they are skipped in both passes and counted in counters[b, 1] (pass 1 only).
#include "common.h"

#include <climits>
#include <type_traits>

namespace iamd {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocksX = 1024;
constexpr int kSeenBit = 1 << 24;

// number of valid leading rows of sample b, clamped to the rows the tensor holds
__device__ __forceinline__ int valid_rows(const int* __restrict__ counts, int64_t cs, int b,
                                          int R) {
  return min(max(counts[b * cs], 0), R);
}

// adds the block's dropped rows to counters[1]: one integer atomic per wave that dropped any
__device__ __forceinline__ void count_drops(int* __restrict__ ctr, int dropped) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) dropped += __shfl_down(dropped, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && dropped) atomicAdd(ctr + 1, dropped);
}

// tensor2im's quantisation: (x + 1) / 2 * 255 as two fp32 roundings (the halving is exact),
// clamped to [0, 255] and truncated. NaN maps to 0.
__device__ __forceinline__ int quantise(float x) {
  float t = __fmul_rn(__fadd_rn(x, 1.f) * 0.5f, 255.f);
  t = t != t ? 0.f : fminf(fmaxf(t, 0.f), 255.f);
  return (int)t;
}

// pass 1 of both operations: win[b, target] = max row number, over the valid rows of sample b.
// kPixel: the target is the pixel (render), else the point id (update).
template <bool kPixel>
__global__ void __launch_bounds__(kThreads)
splat_winner_kernel(const int* __restrict__ rows, int64_t rs, const int* __restrict__ counts,
                    int64_t cs, int* __restrict__ win, int* __restrict__ counters, int R, int P,
                    int H, int W, int bump_call) {
  const int b = blockIdx.y;
  const int n = valid_rows(counts, cs, b, R);
  int* __restrict__ ctr = counters + b * 4;
  if (bump_call && blockIdx.x == 0 && threadIdx.x == 0 && n > 0) ctr[0] += 1;
  const int* __restrict__ rw = rows + b * rs;
  int* __restrict__ wb = win + (int64_t)b * (kPixel ? H * W : P);
  int dropped = 0;
  for (int r = blockIdx.x * kThreads + threadIdx.x; r < n; r += gridDim.x * kThreads) {
    const int i = rw[r * 3], j = rw[r * 3 + 1], pid = rw[r * 3 + 2];
    const bool ok = (unsigned)pid < (unsigned)P && (unsigned)i < (unsigned)H &&
                    (unsigned)j < (unsigned)W;
    if (!ok) {
      ++dropped;
      continue;
    }
    atomicMax(wb + (kPixel ? i * W + j : pid), r);
  }
  count_drops(ctr, dropped);
}

// update pass 2: the winning row of every listed point colours the point if it is unseen
template <typename T>
__global__ void __launch_bounds__(kThreads)
splat_update_kernel(const T* __restrict__ img, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                    const int* __restrict__ rows, int64_t rs, const int* __restrict__ counts,
                    int64_t cs, int* __restrict__ win, int* __restrict__ color,
                    int* __restrict__ seen_time, const int* __restrict__ counters, int R, int P,
                    int H, int W) {
  const int b = blockIdx.y;
  const int n = valid_rows(counts, cs, b, R);
  const int call_idx = counters[b * 4];
  const int* __restrict__ rw = rows + b * rs;
  const int64_t pb = (int64_t)b * P;
  const T* __restrict__ im = img + b * sb;
  for (int r = blockIdx.x * kThreads + threadIdx.x; r < n; r += gridDim.x * kThreads) {
    const int i = rw[r * 3], j = rw[r * 3 + 1], pid = rw[r * 3 + 2];
    if ((unsigned)pid >= (unsigned)P || (unsigned)i >= (unsigned)H || (unsigned)j >= (unsigned)W)
      continue;
    if (win[pb + pid] != r) continue;
    win[pb + pid] = -1;
    if (color[pb + pid] & kSeenBit) continue;
    const T* __restrict__ px = im + i * sh + j * sw;
    const int c0 = quantise(to_f<T>(px[0]));
    const int c1 = quantise(to_f<T>(px[sc]));
    const int c2 = quantise(to_f<T>(px[2 * sc]));
    color[pb + pid] = c0 | (c1 << 8) | (c2 << 16) | kSeenBit;
    seen_time[pb + pid] = call_idx;
  }
}

// (c / 255 - 0.5) * 2 as PyTorch's div / sub / mul compute it in fp32
__device__ __forceinline__ float unquantise(int c) {
  return __fsub_rn(__fdiv_rn((float)c, 255.f), 0.5f) * 2.f;
}

// render pass 2: out[b, 0..3, p .. p + V) for every pixel p; V pixels per thread
template <int V>
__global__ void __launch_bounds__(kThreads)
splat_render_kernel(const int* __restrict__ rows, int64_t rs, int* __restrict__ win,
                    const int* __restrict__ color, float* __restrict__ out, int R, int P,
                    int HW) {
  const int b = blockIdx.y;
  const int* __restrict__ rw = rows + b * rs;
  int* __restrict__ wb = win + (int64_t)b * HW;
  const int* __restrict__ cb = color + (int64_t)b * P;
  float* __restrict__ ob = out + (int64_t)b * 4 * HW;
  const int nv = HW / V;
  for (int t = blockIdx.x * kThreads + threadIdx.x; t < nv; t += gridDim.x * kThreads) {
    Pack<int, V> wr = *reinterpret_cast<const Pack<int, V>*>(wb + t * V);
    float o[4][V];
    bool any = false;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      // a listed pixel shows its point's word (0 while unseen, as the reference's
      // zero-initialised arrays give); an unlisted one the zero image, i.e. word 0 as well
      int word = 0;
      const int r = wr.v[k];
      if (r >= 0 && r < R) {
        any = true;
        const int pid = rw[r * 3 + 2];
        if ((unsigned)pid < (unsigned)P) word = cb[pid];
      }
      o[0][k] = unquantise(word & 255);
      o[1][k] = unquantise((word >> 8) & 255);
      o[2][k] = unquantise((word >> 16) & 255);
      o[3][k] = (word & kSeenBit) ? 1.f : 0.f;
      wr.v[k] = -1;
    }
    if (any) *reinterpret_cast<Pack<int, V>*>(wb + t * V) = wr;
#pragma unroll
    for (int c = 0; c < 4; ++c) store_vec<float, V>(ob + (int64_t)c * HW + t * V, o[c]);
  }
}

struct Rows {
  const int* rows;
  const int* counts;
  int64_t rs, cs;
  int B, R;
};

// rows int32 [B, R, 3] (rows of one sample contiguous, any batch stride) and counts int32 [B]
Rows check_rows(const at::Tensor& rows, const at::Tensor& counts, const at::Tensor& state,
                const char* what) {
  IAMD_CHECK(rows.is_cuda() && rows.scalar_type() == at::kInt && rows.dim() == 3 &&
                 rows.size(2) == 3 && rows.stride(2) == 1 && rows.stride(1) == 3,
             what, ": rows must be an int32 [B, R, 3] CUDA tensor with contiguous samples");
  IAMD_CHECK(counts.is_cuda() && counts.scalar_type() == at::kInt && counts.dim() == 1 &&
                 counts.size(0) == rows.size(0),
             what, ": counts must be an int32 [B] CUDA tensor");
  IAMD_CHECK(rows.size(0) == state.size(0), what, ": batch of rows and state differ");
  IAMD_CHECK(rows.size(1) < INT_MAX / 3, what, ": too many rows");
  IAMD_CHECK(rows.size(0) <= 65535, what, ": batch too large");
  return Rows{rows.data_ptr<int>(), counts.data_ptr<int>(), rows.stride(0), counts.stride(0),
              (int)rows.size(0), (int)rows.size(1)};
}

void check_state(const at::Tensor& t, int64_t B, int64_t n, const char* what, const char* name) {
  IAMD_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.dim() == 2 && t.size(0) == B &&
                 t.size(1) == n && t.is_contiguous(),
             what, ": ", name, " must be a contiguous int32 [", B, ", ", n, "] CUDA tensor");
}

int grid_for(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, kMaxBlocksX));
}

}  // namespace

// Colours the unseen points that rows[b, :counts[b]] list with image[b]'s pixels, in place.
void splat_update(const at::Tensor& image, const at::Tensor& rows, const at::Tensor& counts,
                  at::Tensor& color, at::Tensor& seen_time, at::Tensor& counters,
                  at::Tensor& win_pt) {
  IAMD_CHECK(image.is_cuda() && image.dim() == 4 && image.size(1) == 3,
             "splat_update: [B, 3, H, W] CUDA image expected");
  IAMD_CHECK(image.scalar_type() == at::kBFloat16 || image.scalar_type() == at::kFloat,
             "splat_update: bf16 or fp32 image expected");
  IAMD_CHECK(image.numel() < INT_MAX, "splat_update: image too large");
  const Rows r = check_rows(rows, counts, color, "splat_update");
  const int64_t P = color.size(1);
  IAMD_CHECK(image.size(0) == r.B, "splat_update: batch of image and rows differ");
  IAMD_CHECK(P > 0 && P < INT_MAX, "splat_update: bad point capacity");
  check_state(color, r.B, P, "splat_update", "color");
  check_state(seen_time, r.B, P, "splat_update", "seen_time");
  check_state(win_pt, r.B, P, "splat_update", "win_pt");
  check_state(counters, r.B, 4, "splat_update", "counters");
  if (r.B == 0 || r.R == 0) return;
  const int H = (int)image.size(2), W = (int)image.size(3);
  const dim3 grid(grid_for(r.R), r.B);
  hipLaunchKernelGGL((splat_winner_kernel<false>), grid, dim3(kThreads), 0, stream(), r.rows,
                     r.rs, r.counts, r.cs, win_pt.data_ptr<int>(), counters.data_ptr<int>(), r.R,
                     (int)P, H, W, 1);
  IAMD_LAUNCH_CHECK();
  auto launch = [&](auto tag) {
    using scalar_t = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL((splat_update_kernel<scalar_t>), grid, dim3(kThreads), 0, stream(),
                       reinterpret_cast<const scalar_t*>(image.data_ptr()), image.stride(0),
                       image.stride(1), image.stride(2), image.stride(3), r.rows, r.rs, r.counts,
                       r.cs, win_pt.data_ptr<int>(), color.data_ptr<int>(),
                       seen_time.data_ptr<int>(), counters.data_ptr<int>(), r.R, (int)P, H, W);
  };
  if (image.scalar_type() == at::kFloat)
    launch(static_cast<float*>(nullptr));
  else
    launch(static_cast<__hip_bfloat16*>(nullptr));
  IAMD_LAUNCH_CHECK();
}

// fp32 [B, 4, h, w]: stored colour in [-1, 1] and seen flag of the point each listed pixel
// shows, (-1, -1, -1, 0) elsewhere. win_px: int32 [B, h * w], -1 on entry and on return.
at::Tensor splat_render(const at::Tensor& rows, const at::Tensor& counts, const at::Tensor& color,
                        at::Tensor& counters, at::Tensor& win_px, int64_t h, int64_t w) {
  const Rows r = check_rows(rows, counts, color, "splat_render");
  const int64_t P = color.size(1);
  IAMD_CHECK(h > 0 && w > 0 && h * w < INT_MAX / 4, "splat_render: bad output size");
  IAMD_CHECK(P > 0 && P < INT_MAX, "splat_render: bad point capacity");
  check_state(color, r.B, P, "splat_render", "color");
  check_state(win_px, r.B, h * w, "splat_render", "win_px");
  check_state(counters, r.B, 4, "splat_render", "counters");
  auto out = at::empty({r.B, 4, h, w}, color.options().dtype(at::kFloat));
  if (r.B == 0) return out;
  const int HW = (int)(h * w);
  if (r.R > 0) {
    hipLaunchKernelGGL((splat_winner_kernel<true>), dim3(grid_for(r.R), r.B), dim3(kThreads), 0,
                       stream(), r.rows, r.rs, r.counts, r.cs, win_px.data_ptr<int>(),
                       counters.data_ptr<int>(), r.R, (int)P, (int)h, (int)w, 0);
    IAMD_LAUNCH_CHECK();
  }
  if (HW % 4 == 0) {
    hipLaunchKernelGGL((splat_render_kernel<4>), dim3(grid_for(HW / 4), r.B), dim3(kThreads), 0,
                       stream(), r.rows, r.rs, win_px.data_ptr<int>(), color.data_ptr<int>(),
                       out.data_ptr<float>(), r.R, (int)P, HW);
  } else {
    hipLaunchKernelGGL((splat_render_kernel<1>), dim3(grid_for(HW), r.B), dim3(kThreads), 0,
                       stream(), r.rows, r.rs, win_px.data_ptr<int>(), color.data_ptr<int>(),
                       out.data_ptr<float>(), r.R, (int)P, HW);
  }
  IAMD_LAUNCH_CHECK();
  return out;
}

}  // namespace iamd
