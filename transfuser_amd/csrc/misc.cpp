// Small elementwise kernels, multi-tensor AdamW, LiDAR histogram.
#include "tf_common.h"
#include "tf_hist.h"
#include "../../include/transfuser_hip.h"

using namespace tf;

namespace {

inline int ew_blocks(long n, int cap = 4096) {
    long b = (n + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// out = dy * [y > 0]
__global__ void __launch_bounds__(256) relu_mask_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = (y[i] > 0.f) ? dy[i] : 0.f;
}
// out = alpha * a + beta * b (b optional)
__global__ void __launch_bounds__(256) axpby_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, float alpha,
                                                    float beta, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = alpha * a[i] + (b ? beta * b[i] : 0.f);
}
__global__ void __launch_bounds__(256) sigmoid_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = sigmoidf_(x[i]);
}
// dropout with our counter-based RNG: y = keep ? x / (1-p) : 0 ; same call regenerates the mask in backward
__global__ void __launch_bounds__(256) dropout_kernel(const float* __restrict__ x, float* __restrict__ y, long n, const uint32_t* __restrict__ seed,
                                                      uint32_t site, uint32_t thresh, float keep_scale) {
    const uint32_t sd = *seed;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        y[i] = dropout_keep(sd, site, (uint32_t)i, thresh) ? x[i] * keep_scale : 0.f;
}

// y = res + dropout(x): the residual adds behind resid_drop (transfuser.py:543-544) in one pass; same element -> mask mapping as dropout_kernel
__global__ void __launch_bounds__(256) dropout_add_kernel(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ y, long n,
                                                          const uint32_t* __restrict__ seed, uint32_t site, uint32_t thresh, float keep_scale) {
    const uint32_t sd = *seed;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        y[i] = res[i] + (dropout_keep(sd, site, (uint32_t)i, thresh) ? x[i] * keep_scale : 0.f);
}

// fp32 -> bf16 (round to nearest even) and back with a scale: the optional bf16 gradient buckets of the data-parallel all-reduce
// (336 MB instead of 672 MB over xGMI per step; train.py:134 reduces fp32 - this is an opt-in of this framework)
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));     // Inf / NaN (NaN stays NaN)
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__global__ void __launch_bounds__(256) cast_f32_bf16_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = f32_to_bf16_rne(x[i]);
}
__global__ void __launch_bounds__(256) cast_bf16_f32_kernel(const uint16_t* __restrict__ x, float* __restrict__ y, long n, float scale) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = __uint_as_float((uint32_t)x[i] << 16) * scale;
}

// torch.optim.AdamW (train.py:142: lr 1e-4, betas (.9,.999), eps 1e-8, weight_decay 0.01, decoupled),
// ONE launch over the flat parameter arena.  state[0] = step (float), state[1] = lr; the step is
// advanced by adamw_tick_kernel so a captured graph replays correctly.
__global__ void adamw_tick_kernel(float* state, const float* ls = nullptr) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && !(ls && ls[2] != 0.f)) state[0] += 1.f;      // a skipped (overflowed) step does not count
}
// ---- dynamic loss scaling for the fp16 mode (the reference trains fp32 and has none; semantics of torch.cuda.amp.GradScaler: skip the
// optimizer step when any gradient is non-finite and halve the scale, double it after growth_interval clean steps).  Everything lives on
// the device - ls = {scale, good steps, found_inf, growth interval} - so the captured step replays it: the backward of step t is seeded
// with ls[0] (the Engine's seed tensor IS a view of it), this check reads the finished gradients, AdamW divides by ls[0] or returns, and the
// update kernel prepares ls[0] for step t + 1.
__global__ void __launch_bounds__(256) grad_nonfinite_kernel(const float* __restrict__ g, long n4, long n, float* __restrict__ ls) {
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        bad |= ((__float_as_uint(v.x) & 0x7f800000u) == 0x7f800000u) | ((__float_as_uint(v.y) & 0x7f800000u) == 0x7f800000u) |
               ((__float_as_uint(v.z) & 0x7f800000u) == 0x7f800000u) | ((__float_as_uint(v.w) & 0x7f800000u) == 0x7f800000u);
    }
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) bad |= (__float_as_uint(g[i]) & 0x7f800000u) == 0x7f800000u;
    if (bad) ls[2] = 1.0f;             // every writer stores the same value: no atomic needed
}
__global__ void loss_scale_update_kernel(float* __restrict__ ls) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float scale = ls[0], good = ls[1];
    if (ls[2] != 0.f) { scale = fmaxf(scale * 0.5f, 1.0f); good = 0.f; }
    else if (++good >= ls[3]) { scale = fminf(scale * 2.0f, 16777216.0f); good = 0.f; }
    ls[0] = scale; ls[1] = good; ls[2] = 0.f;
}
// ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_ in front of the optimizer step; the reference's loop, train.py:305-314, has
// none).  Two launches and no pass that rewrites the gradients: grad_sumsq_kernel reads the norm range once and leaves ONE partial sum of squares
// per block in caller scratch (a plain store - no atomics, the block count is a function of n alone, so the sum is a fixed-order sum on every
// device); every block of the clipping instantiation of adamw_kernel re-reduces the <= kSumsqMaxParts partials in its prologue, all in the same
// order (the pattern of pillars.cpp's second statistics pass: no finalize launch), and uses gs * coef where the plain one uses gs.
constexpr int kSumsqMaxParts = 1024;
inline int sumsq_parts(long n) {        // one block per 1024 floats (256 float4 lanes) up to the cap, then grid-stride trips
    const long b = (n + 1023) / 1024;
    return (int)(b < 1 ? 1 : (b > kSumsqMaxParts ? kSumsqMaxParts : b));
}
__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float* __restrict__ g, long n4, long n, float* __restrict__ partials) {
    __shared__ float red[4];
    const long stride = (long)gridDim.x * 256;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;          // one accumulator per float4 component: n / (1024 P) sequential adds each
    for (; i + 3 * stride < n4; i += 4 * stride) {         // four 16-byte loads in flight per thread and trip
        const float4 a = reinterpret_cast<const float4*>(g)[i], b = reinterpret_cast<const float4*>(g)[i + stride];
        const float4 c = reinterpret_cast<const float4*>(g)[i + 2 * stride], d = reinterpret_cast<const float4*>(g)[i + 3 * stride];
        sx += a.x * a.x; sy += a.y * a.y; sz += a.z * a.z; sw += a.w * a.w;
        sx += b.x * b.x; sy += b.y * b.y; sz += b.z * b.z; sw += b.w * b.w;
        sx += c.x * c.x; sy += c.y * c.y; sz += c.z * c.z; sw += c.w * c.w;
        sx += d.x * d.x; sy += d.y * d.y; sz += d.z * d.z; sw += d.w * d.w;
    }
    for (; i < n4; i += stride) {
        const float4 a = reinterpret_cast<const float4*>(g)[i];
        sx += a.x * a.x; sy += a.y * a.y; sz += a.z * a.z; sw += a.w * a.w;
    }
    for (long j = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; j < n; j += stride) sx += g[j] * g[j];      // scalar tail (< 4 elements)
    const float t = block_sum<4>((sx + sy) + (sz + sw), red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
struct ClipArgs { const float* partials; int nparts; float max_norm; float* norm_out; };
// adamw_kernel<> is the plain update (its parameter list and body are what they were before the clipping instantiation existed: the pack is empty
// and the `if constexpr` blocks vanish); adamw_kernel<ClipArgs> takes one more argument and scales the gradients by the clip coefficient as well.
template <class... CLIP>
__global__ void __launch_bounds__(256) adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                    long n4, long n, const float* __restrict__ state, float b1, float b2, float eps, float wd, float gs,
                                                    const float* __restrict__ ls, CLIP... clip) {
    if (ls) {                          // dynamic loss scale: ls = {scale, good steps, found_inf, growth interval}; an overflowed step is skipped as a whole
        if (ls[2] != 0.f) return;      // (nothing is written then, norm_out included)
        if constexpr (sizeof...(CLIP) > 0) gs = gs / ls[0];      // the caller's scale (an accumulation window's 1 / k) composes with 1 / loss scale
        else gs = 1.0f / ls[0];
    }
    if constexpr (sizeof...(CLIP) > 0) {
        __shared__ float red[4];
        const ClipArgs c = (clip, ...);
        float s = 0.f;
        for (int i = threadIdx.x; i < c.nparts; i += 256) s += c.partials[i];      // <= 4 terms per thread in index order, then the block tree: the
        s = block_sum<4>(s, red);                                                   // same order in every block, so every block holds the same bits
        const float norm = gs * sqrtf(s);
        const float r = c.max_norm / (norm + 1e-6f);
        gs *= r > 1.f ? 1.f : r;       // clamp(max = 1) as torch does it: a NaN norm stays a NaN coefficient, an infinite one gives 0
        if (blockIdx.x == 0 && threadIdx.x == 0) c.norm_out[0] = norm;
    }
    const float step = state[0], lr = state[1];
    const float bc1 = 1.f - powf(b1, step), bc2 = 1.f - powf(b2, step);
    const float step_size = lr / bc1, inv_sq_bc2 = 1.f / sqrtf(bc2), decay = 1.f - lr * wd;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            G[k] *= gs;                 // 1 / loss scale (exactly 1.0f in the fp32 / bf16 modes: bit-identical to the unscaled update)
            P[k] *= decay;
            M[k] = b1 * M[k] + (1.f - b1) * G[k];
            V[k] = b2 * V[k] + (1.f - b2) * G[k] * G[k];
            P[k] -= step_size * (M[k] / (sqrtf(V[k]) * inv_sq_bc2 + eps));
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    // tail
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float P = p[i] * decay, G = g[i] * gs;
        float M = b1 * m[i] + (1.f - b1) * G, V = b2 * v[i] + (1.f - b2) * G * G;
        p[i] = P - step_size * (M / (sqrtf(V) * inv_sq_bc2 + eps));
        m[i] = M; v[i] = V;
    }
}

// ---- AdamW parameter groups (torch.optim.AdamW's param_groups; the reference's train.py:142 has one group).  Membership is kept per arena TILE of
// kTileFloats floats (train.py's _ALIGN: the arena starts a new tile wherever two neighbours belong to different groups, so no tile straddles two):
// tile_group[t] = the group of floats [64 t, 64 t + 64), table = [ngroups][{lr_mult, weight_decay, frozen}] floats on the device - values written
// there between two replays of a captured graph take effect without a recapture, like state[1].  A frozen tile is skipped before any load: p, m, v
// are neither read nor written and its gradients never reach the norm.  The two kernels below are separate from adamw_kernel<> / grad_sumsq_kernel
// (whose code stays what it is); with lr_mult = 1 the per-element expression sequence is the plain kernel's, so one default group gives its bits.
constexpr int kTileFloats = 64, kTileVec4 = kTileFloats / 4, kGroupRow = 3;
constexpr int kGroupGridCap = 2048;      // 8 resident blocks of 256 threads per CU x 256 CUs: past 2048 x 1024 floats a block makes further grid-stride trips
__device__ __forceinline__ const float* group_row(const uint8_t* __restrict__ tile_group, const float* __restrict__ table, int ngroups, long vec4) {
    const int id = tile_group[vec4 / kTileVec4];
    return table + kGroupRow * (id < ngroups ? id : ngroups - 1);      // an id past the table reads the last row, never past the allocation
}
__global__ void __launch_bounds__(256) grad_sumsq_groups_kernel(const float* __restrict__ g, long n4, const uint8_t* __restrict__ tile_group,
                                                                const float* __restrict__ table, int ngroups, float* __restrict__ partials) {
    __shared__ float red[4];
    const long stride = (long)gridDim.x * 256;
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;          // grad_sumsq_kernel's accumulators and its order of additions (trip by trip)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += 4 * stride) {
        float4 a[4];
        bool live[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                      // four 16-byte loads in flight from clamped indices, independent of the id -> table chain beside
            const long j = i + u * stride, jj = j < n4 ? j : i;      // them: the selection is applied to the VALUES (a frozen tile's NaN is dropped, not multiplied)
            a[u] = reinterpret_cast<const float4*>(g)[jj];
            live[u] = j < n4 && group_row(tile_group, table, ngroups, jj)[2] == 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (live[u]) { sx += a[u].x * a[u].x; sy += a[u].y * a[u].y; sz += a[u].z * a[u].z; sw += a[u].w * a[u].w; }
    }
    const float t = block_sum<4>((sx + sy) + (sz + sw), red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
template <class... CLIP>
__global__ void __launch_bounds__(256) adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                           long n4, const float* __restrict__ state, float b1, float b2, float eps, float gs,
                                                           const uint8_t* __restrict__ tile_group, const float* __restrict__ table, int ngroups, CLIP... clip) {
    if constexpr (sizeof...(CLIP) > 0) {      // the prologue of adamw_kernel<ClipArgs>: every block re-reduces the partials in one fixed order
        __shared__ float red[4];
        const ClipArgs c = (clip, ...);
        float s = 0.f;
        for (int i = threadIdx.x; i < c.nparts; i += 256) s += c.partials[i];
        s = block_sum<4>(s, red);
        const float norm = gs * sqrtf(s);
        const float r = c.max_norm / (norm + 1e-6f);
        gs *= r > 1.f ? 1.f : r;
        if (blockIdx.x == 0 && threadIdx.x == 0) c.norm_out[0] = norm;
    }
    const float step = state[0], lr = state[1];
    const float bc1 = 1.f - powf(b1, step), bc2 = 1.f - powf(b2, step);
    const float inv_sq_bc2 = 1.f / sqrtf(bc2);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float* row = group_row(tile_group, table, ngroups, i);
        if (row[2] != 0.f) continue;                       // frozen: nothing of this tile is touched
        const float lr_g = lr * row[0];
        const float step_size = lr_g / bc1, decay = 1.f - lr_g * row[1];
        float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            G[k] *= gs;
            P[k] *= decay;
            M[k] = b1 * M[k] + (1.f - b1) * G[k];
            V[k] = b2 * V[k] + (1.f - b2) * G[k] * G[k];
            P[k] -= step_size * (M[k] / (sqrtf(V[k]) * inv_sq_bc2 + eps));
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
}

// LiDAR -> 2-bin BEV histogram (data.py:446-470), integer-exact:
//   valid iff -16 <= x <= 16 and -32 <= y <= 0; xbin = min(floor(8x) + 128, 255), ybin = min(floor(8y) + 256, 255)
//   channel = (z <= -2.3) ? 1 : 0;  out[c][ybin][255 - xbin] = min(count, 5) / 5
// Single pass over the cloud: clear + one-thread-per-point counting with int32 atomics on the output's own storage + in-place
// min(cnt, 5) / 5 (tf_hist.h).  Bit-reproducible (integer counters).
__global__ void __launch_bounds__(256) lidar_hist_count_kernel(const float* __restrict__ pts, const int32_t* __restrict__ npts, int max_pts, int stride,
                                                               int vec4, int* __restrict__ counters) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = npts ? (npts[b] < max_pts ? npts[b] : max_pts) : max_pts;
    const int ic = i < max_pts ? i : max_pts - 1;          // clamped address: the load is unconditional, the predicate applies to the cell
    const float* p = pts + ((long)b * max_pts + ic) * stride;
    float x, y, z;
    if (vec4) { const float4 v = *reinterpret_cast<const float4*>(p); x = v.x; y = v.y; z = v.z; }
    else { x = p[0]; y = p[1]; z = p[2]; }
    const int cell = hist_cell<float>(x, y, z);
    hist_add(counters + (long)b * 2 * 256 * 256, i < n ? cell : -1);
}

// ---- round 6: H1 as ONE launch with the counters in LDS ("LDS reduction + coalesced HBM writes", BASELINE north_star).  A 1024-thread block owns a
// SLAB of one sample's output - 16 grid rows x 256 columns x 2 height bins = 8192 int32 counters = 32 KB of LDS - walks the sample's cloud (512 KB at
// 32768 points: every slab block of the sample re-reads it, which is why all blocks of a sample are placed on ONE XCD (block b runs on XCD b % 8 on
// this part; correctness does not depend on it): the cloud leaves HBM once and the 15 re-reads hit that XCD's L2), counts the points of its slab with
// return-less LDS atomics, and writes its 32 KB of min(count, 5) / 5 as float4 rows.  No global atomics, no counter workspace, the 5 MB output is
// written exactly once: algorithmic traffic (16 B / point + 512 KB / sample).  Sixteen 16-byte point loads in flight per thread and trip.
constexpr int kSlabRows = 16, kSlabs = 256 / kSlabRows;
__global__ void __launch_bounds__(1024) lidar_hist_slab_kernel(const float* __restrict__ pts, const int32_t* __restrict__ npts, int B, int max_pts, int stride,
                                                                int vec4, float* __restrict__ out) {
    __shared__ int cnt[2 * kSlabRows * 256];
    const int tid = threadIdx.x;
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int b = xcd + 8 * (j / kSlabs), slab = j % kSlabs;
    if (b >= B) return;
    const int n = npts ? (npts[b] < max_pts ? npts[b] : max_pts) : max_pts;
    const float* base = pts + (long)b * max_pts * stride;
    constexpr int U = 16;                          // point loads in flight per thread and trip: 32768 points = two round trips of the block
    bool first = true;
    for (int i0 = 0; i0 < n || first; i0 += U * 1024) {
        float px[U], py[U], pz[U];
        if (n > 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {          // clamped addresses: the loads are unconditional, the predicate applies to the cell
                const int i = i0 + tid + 1024 * u;
                const float* p = base + (long)(i < n ? i : n - 1) * stride;
                if (vec4) { const float4 v = *reinterpret_cast<const float4*>(p); px[u] = v.x; py[u] = v.y; pz[u] = v.z; }
                else { px[u] = p[0]; py[u] = p[1]; pz[u] = p[2]; }
            }
        }
        if (first) {                               // the counters are cleared while the first trip's points travel
#pragma unroll
            for (int k = 0; k < 2 * kSlabRows * 256 / 1024; ++k) cnt[tid + 1024 * k] = 0;
            __syncthreads();
            first = false;
        }
        if (n > 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int cell = hist_cell<float>(px[u], py[u], pz[u]);          // ((bin * 256 + row) * 256 + column) of the sample's output, -1 = outside
                const int row = (cell >> 8) & 255;
                if (i0 + tid + 1024 * u < n && cell >= 0 && (row / kSlabRows) == slab)
                    atomicAdd(&cnt[((cell >> 16) * kSlabRows + (row % kSlabRows)) * 256 + (cell & 255)], 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2 * kSlabRows * 256 / 4 / 1024; ++k) {
        const int q = tid + 1024 * k;                       // float4 index inside the slab: [bin][row][64 float4]
        const int bin = q / (kSlabRows * 64), r = (q / 64) % kSlabRows, c4 = q % 64;
        const int* c = cnt + q * 4;
        const float4 v = make_float4((float)(c[0] < 5 ? c[0] : 5) / 5.0f, (float)(c[1] < 5 ? c[1] : 5) / 5.0f, (float)(c[2] < 5 ? c[2] : 5) / 5.0f,
                                     (float)(c[3] < 5 ? c[3] : 5) / 5.0f);
        reinterpret_cast<float4*>(out + (((long)b * 2 + bin) * 256 + slab * kSlabRows + r) * 256)[c4] = v;
    }
}
inline bool hist_slab_on() {
    static const bool on = [] { const char* e = getenv("TF_HIST_SLAB"); return !e || atoi(e) != 0; }();      // A/B switch: 0 = global int32 atomics + finishing pass
    return on;
}
}  // namespace

extern "C" int tf_relu_mask_f32(const float* dy, const float* y, float* out, int64_t n, void* stream) {
    TF_REQUIRE(dy && y && out && n >= 0, "tf_relu_mask_f32: bad arguments");
    if (n == 0) return 0;
    TF_LAUNCH(relu_mask_kernel, dim3(ew_blocks(n)), dim3(256), stream, dy, y, out, (long)n);
    return launch_status("tf_relu_mask_f32");
}
extern "C" int tf_axpby_f32(const float* a, const float* b, float* out, float alpha, float beta, int64_t n, void* stream) {
    TF_REQUIRE(a && out && n >= 0, "tf_axpby_f32: bad arguments");
    if (n == 0) return 0;
    TF_LAUNCH(axpby_kernel, dim3(ew_blocks(n)), dim3(256), stream, a, b, out, alpha, beta, (long)n);
    return launch_status("tf_axpby_f32");
}
// total = sum_i w_i * loss_i over <= 16 scalars that live in separate allocations (train.py:307-311: the 11 weighted detailed losses), and its
// backward d loss_i = w_i * d total: one launch each instead of the ~20 0-dim ATen mul / add launches per direction
namespace {
struct WSumArgs { const float* p[16]; float w[16]; int n; };
__global__ void weighted_sum_kernel(WSumArgs a, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < a.n; ++i) s += a.w[i] * a.p[i][0];      // in index order: the reference's left-to-right Python sum
        out[0] = s;
    }
}
__global__ void weighted_sum_bwd_kernel(WSumArgs a, const float* g, float* out) {
    const int i = threadIdx.x;
    if (blockIdx.x == 0 && i < a.n) out[i] = a.w[i] * (g ? g[0] : 1.f);
}
}  // namespace
extern "C" int tf_weighted_sum_f32(const float* const* terms, const float* weights, int n, float* out, void* stream) {
    TF_REQUIRE(terms && weights && out && n >= 1 && n <= 16, "tf_weighted_sum_f32: 1..16 terms (got %d)", n);
    WSumArgs a;
    for (int i = 0; i < 16; ++i) { a.p[i] = i < n ? terms[i] : nullptr; a.w[i] = i < n ? weights[i] : 0.f; }
    a.n = n;
    for (int i = 0; i < n; ++i) TF_REQUIRE(a.p[i], "tf_weighted_sum_f32: null term %d", i);
    TF_LAUNCH(weighted_sum_kernel, dim3(1), dim3(64), stream, a, out);
    return launch_status("tf_weighted_sum_f32");
}
extern "C" int tf_weighted_sum_bwd_f32(const float* dtotal, const float* weights, int n, float* dterms, void* stream) {
    TF_REQUIRE(weights && dterms && n >= 1 && n <= 16, "tf_weighted_sum_bwd_f32: 1..16 terms (got %d)", n);
    WSumArgs a;
    for (int i = 0; i < 16; ++i) { a.p[i] = nullptr; a.w[i] = i < n ? weights[i] : 0.f; }
    a.n = n;
    TF_LAUNCH(weighted_sum_bwd_kernel, dim3(1), dim3(64), stream, a, dtotal, dterms);
    return launch_status("tf_weighted_sum_bwd_f32");
}
extern "C" int tf_sigmoid_f32(const float* x, float* y, int64_t n, void* stream) {
    TF_REQUIRE(x && y && n >= 0, "tf_sigmoid_f32: bad arguments");
    if (n == 0) return 0;
    TF_LAUNCH(sigmoid_kernel, dim3(ew_blocks(n)), dim3(256), stream, x, y, (long)n);
    return launch_status("tf_sigmoid_f32");
}
extern "C" int tf_dropout_f32(const float* x, float* y, int64_t n, const uint32_t* seed_dev, uint32_t site, float p, void* stream) {
    TF_REQUIRE(x && y && seed_dev && n >= 0 && p >= 0.f && p < 1.f, "tf_dropout_f32: bad arguments");
    if (n == 0) return 0;
    const uint32_t thresh = (uint32_t)((double)p * 4294967296.0);
    TF_LAUNCH(dropout_kernel, dim3(ew_blocks(n)), dim3(256), stream, x, y, (long)n, seed_dev, site, thresh, 1.f / (1.f - p));
    return launch_status("tf_dropout_f32");
}
extern "C" int tf_dropout_add_f32(const float* x, const float* res, float* y, int64_t n, const uint32_t* seed_dev, uint32_t site, float p, void* stream) {
    TF_REQUIRE(x && res && y && seed_dev && n >= 0 && p >= 0.f && p < 1.f, "tf_dropout_add_f32: bad arguments");
    if (n == 0) return 0;
    const uint32_t thresh = (uint32_t)((double)p * 4294967296.0);
    TF_LAUNCH(dropout_add_kernel, dim3(ew_blocks(n)), dim3(256), stream, x, res, y, (long)n, seed_dev, site, thresh, 1.f / (1.f - p));
    return launch_status("tf_dropout_add_f32");
}
extern "C" int tf_cast_f32_bf16(const float* x, uint16_t* y, int64_t n, void* stream) {
    TF_REQUIRE(x && y && n >= 0, "tf_cast_f32_bf16: bad arguments");
    if (n == 0) return 0;
    TF_LAUNCH(cast_f32_bf16_kernel, dim3(ew_blocks(n)), dim3(256), stream, x, y, (long)n);
    return launch_status("tf_cast_f32_bf16");
}
extern "C" int tf_cast_bf16_f32(const uint16_t* x, float* y, int64_t n, float scale, void* stream) {
    TF_REQUIRE(x && y && n >= 0, "tf_cast_bf16_f32: bad arguments");
    if (n == 0) return 0;
    TF_LAUNCH(cast_bf16_f32_kernel, dim3(ew_blocks(n)), dim3(256), stream, x, y, (long)n, scale);
    return launch_status("tf_cast_bf16_f32");
}
extern "C" int tf_adamw_scaled_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps,
                                   float weight_decay, float grad_scale, void* stream);
extern "C" int tf_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps,
                            float weight_decay, void* stream) {
    return tf_adamw_scaled_f32(p, g, m, v, n, state_dev, beta1, beta2, eps, weight_decay, 1.0f, stream);
}
extern "C" int tf_adamw_scaled_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps,
                                   float weight_decay, float grad_scale, void* stream) {
    TF_REQUIRE(p && g && m && v && state_dev && n >= 0, "tf_adamw_f32: bad arguments");
    TF_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), "tf_adamw_f32: arenas must be 16-byte aligned");
    TF_LAUNCH(adamw_tick_kernel, dim3(1), dim3(64), stream, state_dev, (const float*)nullptr);
    if (n > 0) TF_LAUNCH(adamw_kernel<>, dim3(ew_blocks(n / 4 + 1, 8192)), dim3(256), stream, p, g, m, v, (long)(n / 4), (long)n, (const float*)state_dev,
                         beta1, beta2, eps, weight_decay, grad_scale, (const float*)nullptr);
    return launch_status("tf_adamw_f32");
}
extern "C" int tf_adamw_dynscale_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps,
                                     float weight_decay, const float* g_check, int64_t n_check, float* ls_state, void* stream) {
    TF_REQUIRE(p && g && m && v && state_dev && ls_state && n >= 0 && n_check >= 0 && (n_check == 0 || g_check), "tf_adamw_dynscale_f32: bad arguments");
    TF_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (!g_check || aligned16(g_check)), "tf_adamw_dynscale_f32: arenas must be 16-byte aligned");
    if (n_check > 0) TF_LAUNCH(grad_nonfinite_kernel, dim3(ew_blocks(n_check / 4 + 1, 8192)), dim3(256), stream, g_check, (long)(n_check / 4), (long)n_check, ls_state);
    TF_LAUNCH(adamw_tick_kernel, dim3(1), dim3(64), stream, state_dev, (const float*)ls_state);
    if (n > 0) TF_LAUNCH(adamw_kernel<>, dim3(ew_blocks(n / 4 + 1, 8192)), dim3(256), stream, p, g, m, v, (long)(n / 4), (long)n, (const float*)state_dev,
                         beta1, beta2, eps, weight_decay, 1.0f, (const float*)ls_state);
    TF_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), stream, ls_state);
    return launch_status("tf_adamw_dynscale_f32");
}
extern "C" int tf_grad_sumsq_parts(int64_t n) { return sumsq_parts((long)n); }
extern "C" int tf_grad_sumsq_f32(const float* g, int64_t n, float* partials, void* stream) {
    TF_REQUIRE(g && partials && n >= 1, "tf_grad_sumsq_f32: bad arguments");
    TF_REQUIRE(aligned16(g), "tf_grad_sumsq_f32: the range must be 16-byte aligned");
    TF_LAUNCH(grad_sumsq_kernel, dim3(sumsq_parts((long)n)), dim3(256), stream, g, (long)(n / 4), (long)n, partials);
    return launch_status("tf_grad_sumsq_f32");
}
extern "C" int tf_adamw_clip_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps,
                                 float weight_decay, float grad_scale, const float* g_norm, int64_t n_norm, const float* partials, int nparts,
                                 float max_norm, float* norm_out, float* ls_state, void* stream) {
    TF_REQUIRE(p && g && m && v && state_dev && partials && norm_out && n >= 0 && n_norm >= 1 && (!ls_state || g_norm), "tf_adamw_clip_f32: bad arguments");
    TF_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (!g_norm || aligned16(g_norm)), "tf_adamw_clip_f32: arenas must be 16-byte aligned");
    TF_REQUIRE(nparts == sumsq_parts((long)n_norm), "tf_adamw_clip_f32: %d partials for a norm range of %ld floats (tf_grad_sumsq_parts gives %d)", nparts,
               (long)n_norm, sumsq_parts((long)n_norm));
    TF_REQUIRE(max_norm > 0.f, "tf_adamw_clip_f32: max_norm must be positive (got %g)", (double)max_norm);
    if (ls_state) TF_LAUNCH(grad_nonfinite_kernel, dim3(ew_blocks(n_norm / 4 + 1, 8192)), dim3(256), stream, g_norm, (long)(n_norm / 4), (long)n_norm, ls_state);
    TF_LAUNCH(adamw_tick_kernel, dim3(1), dim3(64), stream, state_dev, (const float*)ls_state);
    if (n > 0) TF_LAUNCH(adamw_kernel<ClipArgs>, dim3(ew_blocks(n / 4 + 1, 8192)), dim3(256), stream, p, g, m, v, (long)(n / 4), (long)n, (const float*)state_dev,
                         beta1, beta2, eps, weight_decay, grad_scale, (const float*)ls_state, ClipArgs{partials, nparts, max_norm, norm_out});
    if (ls_state) TF_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), stream, ls_state);
    return launch_status("tf_adamw_clip_f32");
}
// ---- parameter groups (include/transfuser_hip.h): the arguments the two entries share are checked in one place
namespace {
inline int groups_args_ok(const char* who, int64_t n, const uint8_t* tile_group, const float* table, int ngroups) {
    TF_REQUIRE(n >= kTileFloats && n % kTileFloats == 0, "%s: the range must be whole %d-float tiles (got %ld floats)", who, kTileFloats, (long)n);
    TF_REQUIRE(tile_group && table, "%s: tile_group and the group table must not be NULL", who);
    TF_REQUIRE(ngroups >= 1 && ngroups <= 255, "%s: 1..255 groups (got %d)", who, ngroups);
    return 0;
}
}  // namespace
extern "C" int tf_grad_sumsq_groups_f32(const float* g, int64_t n, const uint8_t* tile_group, const float* table, int ngroups, float* partials, void* stream) {
    TF_REQUIRE(g && partials, "tf_grad_sumsq_groups_f32: bad arguments");
    TF_REQUIRE(aligned16(g), "tf_grad_sumsq_groups_f32: the range must be 16-byte aligned");
    if (const int rc = groups_args_ok("tf_grad_sumsq_groups_f32", n, tile_group, table, ngroups)) return rc;
    TF_LAUNCH(grad_sumsq_groups_kernel, dim3(sumsq_parts((long)n)), dim3(256), stream, g, (long)(n / 4), tile_group, table, ngroups, partials);
    return launch_status("tf_grad_sumsq_groups_f32");
}
extern "C" int tf_adamw_groups_f32(float* p, const float* g, float* m, float* v, int64_t n, float* state_dev, float beta1, float beta2, float eps,
                                   float grad_scale, const uint8_t* tile_group, const float* table, int ngroups, const float* partials, int nparts,
                                   int64_t n_norm, float max_norm, float* norm_out, void* stream) {
    TF_REQUIRE(p && g && m && v && state_dev, "tf_adamw_groups_f32: bad arguments");
    TF_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), "tf_adamw_groups_f32: arenas must be 16-byte aligned");
    if (const int rc = groups_args_ok("tf_adamw_groups_f32", n, tile_group, table, ngroups)) return rc;
    if (partials) {
        TF_REQUIRE(norm_out && n_norm >= 1, "tf_adamw_groups_f32: clipping needs norm_out and the norm range's size");
        TF_REQUIRE(nparts == sumsq_parts((long)n_norm), "tf_adamw_groups_f32: %d partials for a norm range of %ld floats (tf_grad_sumsq_parts gives %d)", nparts,
                   (long)n_norm, sumsq_parts((long)n_norm));
        TF_REQUIRE(max_norm > 0.f, "tf_adamw_groups_f32: max_norm must be positive (got %g)", (double)max_norm);
    }
    const dim3 grid(ew_blocks(n / 4, kGroupGridCap));
    TF_LAUNCH(adamw_tick_kernel, dim3(1), dim3(64), stream, state_dev, (const float*)nullptr);
    if (partials) TF_LAUNCH(adamw_groups_kernel<ClipArgs>, grid, dim3(256), stream, p, g, m, v, (long)(n / 4), (const float*)state_dev, beta1, beta2, eps, grad_scale,
                            tile_group, table, ngroups, ClipArgs{partials, nparts, max_norm, norm_out});
    else TF_LAUNCH(adamw_groups_kernel<>, grid, dim3(256), stream, p, g, m, v, (long)(n / 4), (const float*)state_dev, beta1, beta2, eps, grad_scale, tile_group,
                   table, ngroups);
    return launch_status("tf_adamw_groups_f32");
}
extern "C" int tf_lidar_hist_f32(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, float* out, void* stream) {
    TF_REQUIRE(points && out && B > 0 && max_points >= 0 && point_stride >= 3, "tf_lidar_hist_f32: bad arguments");
    TF_REQUIRE(aligned16(out), "tf_lidar_hist_f32: out must be 16-byte aligned");
    const long n4 = (long)B * 2 * 256 * 256 / 4;
    if (hist_slab_on()) {
        const int vec4 = (point_stride == 4 && aligned16(points)) ? 1 : 0;
        TF_LAUNCH(lidar_hist_slab_kernel, dim3(8 * cdiv(B, 8) * kSlabs), dim3(1024), stream, points, num_points, B, max_points, point_stride, vec4, out);
        return launch_status("tf_lidar_hist_f32");
    }
    TF_LAUNCH(hist_clear_kernel, dim3(cdiv(n4, 256)), dim3(256), stream, reinterpret_cast<float4*>(out), n4);
    if (max_points > 0) {
        const int vec4 = (point_stride == 4 && aligned16(points)) ? 1 : 0;
        TF_LAUNCH(lidar_hist_count_kernel, dim3(cdiv(max_points, 256), B), dim3(256), stream, points, num_points, max_points, point_stride, vec4,
                  reinterpret_cast<int*>(out));
    }
    TF_LAUNCH(hist_finish_kernel, dim3(cdiv(n4, 256)), dim3(256), stream, reinterpret_cast<float4*>(out), n4);
    return launch_status("tf_lidar_hist_f32");
}
// the same in TWO launches: the counters live in a caller-owned workspace that is all zero on entry and left all zero (tf_hist.h)
extern "C" long tf_lidar_hist_ws_bytes(int B) { return (long)B * 2 * 256 * 256 * 4; }
extern "C" int tf_lidar_hist_ws_f32(const float* points, const int32_t* num_points, int B, int max_points, int point_stride, void* zero_ws, float* out, void* stream) {
    TF_REQUIRE(points && out && zero_ws && B > 0 && max_points >= 0 && point_stride >= 3, "tf_lidar_hist_ws_f32: bad arguments");
    TF_REQUIRE(aligned16(out) && aligned16(zero_ws), "tf_lidar_hist_ws_f32: out / workspace must be 16-byte aligned");
    const long n4 = (long)B * 2 * 256 * 256 / 4;
    if (hist_slab_on()) {       // one launch, counters in LDS: the workspace is not touched (it stays all zero)
        const int vec4 = (point_stride == 4 && aligned16(points)) ? 1 : 0;
        TF_LAUNCH(lidar_hist_slab_kernel, dim3(8 * cdiv(B, 8) * kSlabs), dim3(1024), stream, points, num_points, B, max_points, point_stride, vec4, out);
        return launch_status("tf_lidar_hist_ws_f32");
    }
    if (max_points > 0) {
        const int vec4 = (point_stride == 4 && aligned16(points)) ? 1 : 0;
        TF_LAUNCH(lidar_hist_count_kernel, dim3(cdiv(max_points, 256), B), dim3(256), stream, points, num_points, max_points, point_stride, vec4,
                  reinterpret_cast<int*>(zero_ws));
    }
    TF_LAUNCH(hist_finish_ws_kernel, dim3(cdiv(n4, 256)), dim3(256), stream, reinterpret_cast<int4*>(zero_ws), reinterpret_cast<float4*>(out), n4);
    return launch_status("tf_lidar_hist_ws_f32");
}
