// resolve_plan: which kernel runs a dense contraction and how K is partitioned - decided here, once, for the launch (tf_gemm_engine.h:launch_gemm)
// and for the scratch queries of the sites (tf_gemm_splitk_ws_floats, tf_conv2d_wgrad_ws_floats, tf_stem_conv_wgrad_ws_floats) alike.
#include "tf_gemm_engine.h"

namespace tf {

// plans are tuned per compute precision (fp16 shares the bf16 plans) and per kind of epilogue: store, accumulate, pure accumulation (may split K)
static bool pure_accumulation(const PlanCall& c) { return c.allow_splitk && c.mode == 1 && !c.bias && !c.res && !c.relu; }
static int acc_key(const PlanCall& c) { return (c.mode != 0 ? (pure_accumulation(c) ? 2 : 1) : 0) + 4 * (gemm_precision() == 3 ? 1 : gemm_precision()); }

int heuristic_splitk(int M, int N, int K, int batch, int bm, int bn, int bk) {
    const long tiles = (long)cdiv(M, bm) * cdiv(N, bn) * batch;
    const int ktiles = cdiv(K, bk);
    if (tiles >= 512 || ktiles * bk < 256) return 1;
    long want = (1024 + tiles - 1) / tiles;
    long maxs = (long)ktiles * bk / 128;
    if (want > maxs) want = maxs;
    return want < 1 ? 1 : (int)want;
}

// Heuristic tile choice (used when no tuned plan exists): smallest BN that covers N with the least padding,
// BM=64 when the grid would not fill the 256 CUs, split-K (atomic epilogue) for skinny outputs with deep reductions.
GemmPlan plan_gemm(int M, int N, int K, int batch, bool allow_splitk) {
    int bm = 128, bn;
    if (N <= 32) bn = 32;
    else if (N <= 64) bn = 64;
    else if (N <= 96) bn = 96;
    else {
        const long w128 = (long)cdiv(N, 128) * 128, w96 = (long)cdiv(N, 96) * 96;
        bn = (w96 < w128) ? 96 : 128;
    }
    const long t128 = (long)cdiv(M, 128) * cdiv(N, bn) * batch;
    if ((bn == 128 || bn == 64) && t128 < 384 && M > 64) bm = 64;
    return atomic_plan(bm, bn, 16, 0, allow_splitk ? heuristic_splitk(M, N, K, batch, bm, bn, 16) : 1);
}

// eligibility of the two-pass split for this call: plain row-major single-batch output and enough caller scratch for S slices
// (the tuned two-pass plans stop at 4 slices)
bool twopass_ok(const PlanCall& c, int S, int smax) {
    return c.ws && c.batch == 1 && c.ldcj == 1 && (c.mode == 0 || c.mode == 1) && S >= 2 && S <= smax && (long)S * c.M * twopass_ldws(c.N) <= c.ws_floats;
}

// Deterministic mode (tf_set_deterministic): k-slices of the ORDERED SLAB split that replaces a plan's atomic k-split - slice s stores its raw
// partial tile at sk_ws + s * M * ldws with plain stores, launch_splitk_fixup adds the slices to C in slice order.  The plan's own slice count,
// lowered until the caller's scratch holds that many slices; 1 (unsplit) without scratch, for batched calls and column-strided outputs.
constexpr int kSlabMax = 1 << 16;
static int slab_slices(const PlanCall& c, int splitk) {
    if (!c.ws || c.batch != 1 || c.ldcj != 1 || c.mode != 1 || splitk < 2) return 1;
    const long fit = c.ws_floats / ((long)c.M * twopass_ldws(c.N));
    const long S = splitk < fit ? splitk : fit;
    return S < 2 ? 1 : (int)(S < kSlabMax ? S : kSlabMax);
}

// workgroups of a stream-K launch of this configuration, 0 = not eligible: single-batch, non-atomic epilogue, caller scratch + flags, at least one
// whole tile of work per workgroup (so a tile is cut at most once) and a tile count that does NOT already divide evenly over the resident slots
int streamk_blocks(const PlanCall& c, const DmaKindInfo& ki) {
    if (!c.dma_ok || ki.bm == 0 || !c.ws || !c.flags || c.batch != 1 || c.mode == 2 || c.K < 8 * ki.bk) return 0;
    int per_cu = ki.occ * 4 / ki.nw;                           // __launch_bounds__(64 nw, occ): occ waves per SIMD
    const int by_lds = (160 * 1024) / (ki.lds > 0 ? ki.lds : 1);
    if (per_cu > by_lds) per_cu = by_lds;
    if (per_cu < 1) per_cu = 1;
    const long nt = (long)cdiv(c.M, ki.bm) * cdiv(c.N, ki.bn);
    long P = (long)device_cus() * per_cu;
    if (P > kStreamKMaxBlocks) P = kStreamKMaxBlocks;
    if (P > nt) P = nt;
    P &= ~7L;                                                  // XCD-contiguous positions
    if (P < 8 || nt % P == 0) return 0;                        // already balanced: the data-parallel launch is the same thing without the bookkeeping
    if (P * (long)ki.bm * ki.bn > c.ws_floats) return 0;
    return (int)P;
}
// what a caller brings for a stream-K plan: <= 512 resident workgroups x one 128 x 128 partial tile (larger launches use smaller tiles)
constexpr long kStreamKWsFloats = (long)kStreamKMaxBlocks / 4 * 128 * 128;

ResolvedPlan resolve_plan(const PlanCall& c) {
    ResolvedPlan r;
    GemmPlan& p = r.plan;
    r.sk_ok = pure_accumulation(c);         // split-K only for pure accumulations (weight gradients into the grad arena)
    r.stat = c.stat; r.atomic = false; r.tune = false;
    const bool det = deterministic();       // tf_set_deterministic: no atomic k-split, no tuning (the plan cache records nothing found under the flag)
    // the plan: pinned by a test, else cached (loaded or tuned), else the heuristic one
    if (!forced_plan(&p) && !plan_lookup(c.site, c.M, c.N, c.K, c.batch, acc_key(c), &p)) {
        r.tune = autotune_enabled() && !det;
        p = plan_gemm(c.M, c.N, c.K, c.batch, r.sk_ok);
    }
    auto unsplit = [&p] { p.split = KSplit::None; p.slices = 1; };
    // stream-K: needs an LDS-DMA kind, this call's scratch + flags and a tile count that does not divide over the slots
    if (p.split == KSplit::StreamK) {
        p.slices = p.kind >= 1 ? streamk_blocks(c, dma_kind_info(p.kind)) : 0;
        if (p.slices == 0) unsplit();
    }
    if (r.stat) {
        // fused output statistics need the whole reduction in one block: no k-split - but the owner of a stream-K tile holds the complete sum
        // (statistics as usual), and a cached two-pass plan keeps its speed and reports "no statistics" (nparts 0): the caller runs its separate
        // reduction for this (rare: <= 256-tile) output
        if (p.split == KSplit::StreamK) {}
        else if (p.split == KSplit::TwoPass && p.kind >= 1 && twopass_ok(c, p.slices)) r.stat = false;
        else unsplit();
        if (c.mode != 0 || c.res || c.relu || c.mask) r.stat = false;
    }
    if (p.split == KSplit::TwoPass) {
        if (p.kind < 1 || !twopass_ok(c, p.slices) || !c.dma_ok) unsplit();       // no scratch on this call / not a plain output / the register-staged kernels run instead
    } else if (p.split == KSplit::Atomic) {
        if (!r.sk_ok) unsplit();
        else if (det) {                     // the plan's tile and slice count, the slices combined in slice order through the caller's scratch
            p.slices = c.slab_layout ? slab_slices(c, p.slices) : 1;
            if (p.slices < 2) unsplit(); else p.split = KSplit::Slab;
        } else r.atomic = true;
    }
    const long slice = (long)c.M * twopass_ldws(c.N);
    r.ws_floats = p.split == KSplit::StreamK ? kStreamKWsFloats : (p.split == KSplit::TwoPass || p.split == KSplit::Slab) ? p.slices * slice : 0;
    return r;
}

void store_tuned_plan(const PlanCall& c, const GemmPlan& p) { plan_store(c.site, c.M, c.N, c.K, c.batch, acc_key(c), p); }

long plan_scratch_floats(PlanCall c) {
    c.ws = c.flags = true; c.ws_floats = 0x7fffffffffffffffL;
    const ResolvedPlan r = resolve_plan(c);
    if (!r.tune) return r.ws_floats;
    // autotuner on: its two-pass and stream-K candidates (LDS-DMA kernels, row-major single-batch output) need scratch to be tried at all - the
    // four-slice maximum
    if (!c.dma_ok || c.batch != 1 || c.ldcj != 1) return 0;
    const long four = 4L * c.M * twopass_ldws(c.N);
    return four > kStreamKWsFloats ? four : kStreamKWsFloats;
}

}  // namespace tf
