// Exponential moving average (EMA) of the weights, and the in-place exchange that puts the averaged values where the modules read them.
// The reference keeps no average (its optimizer and checkpoint code, train.py:142,204-210,381-384, is what this sits beside); the semantics are
// timm's ModelEmaV2 (e += (1 - decay) * (p - e), initialised by a copy) with ModelEmaV3's optional warm-up decay = min(decay, (1 + n) / (10 + n)).
// The average is a pass of its OWN behind the optimizer step - adamw_kernel<> / adamw_groups_kernel<> are untouched - at 12 B per parameter
// (p read, e read, e written) against AdamW's 28.  Everything here is element-wise: no atomics, no workspace, nothing allocated, capturable,
// legal under tf_set_deterministic(1).
//
// ema_state = {decay, num_updates, last_opt_step, coef} floats on the device (like AdamW's {step, lr}): ema_tick_kernel - one thread, a launch
// of its own in front of the apply kernels for the reason adamw_tick_kernel is one - decides whether this step updates and leaves coef = 1 - d
// or 0; the apply kernels only READ the state, so no block reads a word another block of the same launch writes.
#include "tf_common.h"
#include "../../include/transfuser_hip.h"

using namespace tf;

namespace {

constexpr int kEmaGridCap = 2048;      // adamw_groups_kernel's grid policy (misc.cpp kGroupGridCap): 8 resident blocks of 256 threads per CU x 256 CUs
constexpr int kMultiRows = 2;          // blocks per table entry (a column of the grid): the largest BatchNorm vector, 1512 floats, is three trips each

inline int ema_blocks(long n4) {
    long b = (n4 + 255) / 256;
    if (b > kEmaGridCap) b = kEmaGridCap;
    if (b < 1) b = 1;
    return (int)b;
}

// opt = FlatAdamW's {step, lr} (nullable).  adamw_tick_kernel does not count an overflowed fp16 step, so "the optimizer's step counter did not
// move since the last update" IS "the step was skipped": the average skips it too, without reading the loss-scale state.
__global__ void ema_tick_kernel(float* __restrict__ st, const float* __restrict__ opt, int every, int warmup) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float t = st[2];
    if (opt) {
        t = opt[0];
        if (t == st[2] || fmodf(t, (float)every) != 0.f) { st[3] = 0.f; return; }
    }
    const float decay = st[0], n = st[1];
    const float w = (1.f + n) / (10.f + n);
    const float d = (warmup && w < decay) ? w : decay;
    st[3] = 1.f - d;
    st[1] = n + 1.f;
    st[2] = t;
}

// e = fma(coef, p - e, e) over n4 float4 lanes
__global__ void __launch_bounds__(256) ema_apply_kernel(float* __restrict__ e, const float* __restrict__ p, long n4, const float* __restrict__ st) {
    const float coef = st[3];
    if (coef == 0.f) return;           // no update this step: nothing is read, nothing is written
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 ee = reinterpret_cast<float4*>(e)[i];
        const float4 pp = reinterpret_cast<const float4*>(p)[i];
        ee.x = fmaf(coef, pp.x - ee.x, ee.x);
        ee.y = fmaf(coef, pp.y - ee.y, ee.y);
        ee.z = fmaf(coef, pp.z - ee.z, ee.z);
        ee.w = fmaf(coef, pp.w - ee.w, ee.w);
        reinterpret_cast<float4*>(e)[i] = ee;
    }
}

// the same expression over a table of small vectors (the module buffers outside the arena): block column blockIdx.x owns entry blockIdx.x
__global__ void __launch_bounds__(256) ema_apply_multi_kernel(const tf_ema_item* __restrict__ items, const float* __restrict__ st) {
    const float coef = st[3];
    if (coef == 0.f) return;
    const tf_ema_item it = items[blockIdx.x];
    for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < it.count; i += (long)gridDim.y * 256) {
        const float ee = it.ema[i];
        it.ema[i] = fmaf(coef, it.live[i] - ee, ee);
    }
}

__global__ void __launch_bounds__(256) swap_kernel(float* __restrict__ a, float* __restrict__ b, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 aa = reinterpret_cast<float4*>(a)[i], bb = reinterpret_cast<float4*>(b)[i];
        reinterpret_cast<float4*>(a)[i] = bb;
        reinterpret_cast<float4*>(b)[i] = aa;
    }
}

__global__ void __launch_bounds__(256) swap_multi_kernel(const tf_ema_item* __restrict__ items) {
    const tf_ema_item it = items[blockIdx.x];
    for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < it.count; i += (long)gridDim.y * 256) {
        const float aa = it.ema[i], bb = it.live[i];
        it.ema[i] = bb;
        it.live[i] = aa;
    }
}

}  // namespace

extern "C" int tf_ema_tick_f32(float* ema_state, const float* opt_state, int every, int warmup, void* stream) {
    TF_REQUIRE(ema_state, "tf_ema_tick_f32: ema_state must not be NULL");
    TF_REQUIRE(every >= 1, "tf_ema_tick_f32: every must be >= 1 (got %d)", every);
    TF_LAUNCH(ema_tick_kernel, dim3(1), dim3(64), stream, ema_state, opt_state, every, warmup ? 1 : 0);
    return launch_status("tf_ema_tick_f32");
}

extern "C" int tf_ema_apply_f32(float* ema, const float* p, int64_t n, const float* ema_state, void* stream) {
    TF_REQUIRE(ema && p && ema_state && n >= 0, "tf_ema_apply_f32: bad arguments");
    TF_REQUIRE(n % 4 == 0, "tf_ema_apply_f32: the range must be whole float4 lanes (got %ld floats)", (long)n);
    TF_REQUIRE(aligned16(ema) && aligned16(p), "tf_ema_apply_f32: ranges must be 16-byte aligned");
    TF_REQUIRE(ema + n <= p || p + n <= ema || n == 0, "tf_ema_apply_f32: the two ranges overlap");
    if (n > 0) TF_LAUNCH(ema_apply_kernel, dim3(ema_blocks(n / 4)), dim3(256), stream, ema, p, (long)(n / 4), ema_state);
    return launch_status("tf_ema_apply_f32");
}

extern "C" int tf_ema_apply_multi_f32(const tf_ema_item* table_dev, int nentries, const float* ema_state, void* stream) {
    TF_REQUIRE(table_dev && ema_state, "tf_ema_apply_multi_f32: bad arguments");
    TF_REQUIRE(nentries >= 1, "tf_ema_apply_multi_f32: nentries must be >= 1 (got %d)", nentries);
    TF_LAUNCH(ema_apply_multi_kernel, dim3(nentries, kMultiRows), dim3(256), stream, table_dev, ema_state);
    return launch_status("tf_ema_apply_multi_f32");
}

extern "C" int tf_swap_f32(float* a, float* b, int64_t n, void* stream) {
    TF_REQUIRE(a && b && n >= 0, "tf_swap_f32: bad arguments");
    TF_REQUIRE(n % 4 == 0, "tf_swap_f32: the range must be whole float4 lanes (got %ld floats)", (long)n);
    TF_REQUIRE(aligned16(a) && aligned16(b), "tf_swap_f32: ranges must be 16-byte aligned");
    TF_REQUIRE(a + n <= b || b + n <= a || n == 0, "tf_swap_f32: the two ranges overlap");
    if (n > 0) TF_LAUNCH(swap_kernel, dim3(ema_blocks(n / 4)), dim3(256), stream, a, b, (long)(n / 4));
    return launch_status("tf_swap_f32");
}

extern "C" int tf_swap_multi_f32(const tf_ema_item* table_dev, int nentries, void* stream) {
    TF_REQUIRE(table_dev, "tf_swap_multi_f32: bad arguments");
    TF_REQUIRE(nentries >= 1, "tf_swap_multi_f32: nentries must be >= 1 (got %d)", nentries);
    TF_LAUNCH(swap_multi_kernel, dim3(nentries, kMultiRows), dim3(256), stream, table_dev);
    return launch_status("tf_swap_multi_f32");
}
