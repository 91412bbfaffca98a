// Convolution weight gradient as implicit GEMM on the MFMA engine (contraction over the output pixels; im2col loader on the B side).
#include "tf_gemm_engine.h"
#include "../../include/transfuser_hip.h"
#include "conv_common.h"

using namespace tf;

// Few output channels per group (RegNet group width 24, decoder / head tails with 32, 7, 1): compute dW^T - rows = (tap, ci), cols = co - so Cog
// sits in a 32-wide column tile instead of a 128-row tile.  Not for a deterministic one-group accumulation: the slab split needs a row-major
// output, so the unswapped orientation is kept (grouped calls run unsplit either way).
static bool wgrad_swapped(const tf_conv_geom* g, int accumulate) { return g->Cout / g->groups <= 32 && !(deterministic() && accumulate && g->groups == 1); }
static const char* wgrad_site(bool swapped) { return swapped ? "tf_conv2d_wgrad_f32[swapped]" : "tf_conv2d_wgrad_f32"; }
// the epilogue of the call, as the launch uses it and as the scratch query describes it to resolve_plan()
static GemmEpi wgrad_epi(const tf_conv_geom* g, float* dw, int accumulate, float* ws, long ws_floats, bool swapped) {
    const int Cog = g->Cout / g->groups, Ncols = g->ksize * g->ksize * (g->Cin / g->groups);
    GemmEpi ep;
    ep.C = dw; ep.ldc = Ncols; ep.ldcj = 1; ep.sc_outer = 0; ep.sc_inner = (long)Cog * Ncols; ep.inner = g->groups; ep.bias = nullptr; ep.sbias = 0;
    ep.res = nullptr; ep.ldres = 0; ep.alpha = 1.f; ep.relu = 0; ep.mode = accumulate ? 1 : 0;
    ep.sk_ws = ws; ep.sk_ws_floats = ws ? ws_floats : 0;      // the ordered slab k-split of the deterministic mode; unused otherwise
    if (swapped) { ep.ldc = 1; ep.ldcj = Ncols; }
    return ep;
}

static int conv2d_wgrad(const tf_conv_geom* g, const float* dy, const float* x, float* dw, int accumulate, float* ws, long ws_floats, void* stream) {
    if (int e = check_geom(g, "tf_conv2d_wgrad_f32")) return e;
    const int Cig = g->Cin / g->groups, Cog = g->Cout / g->groups, taps = g->ksize * g->ksize;
    const int Mred = g->B * g->Ho * g->Wo, Ncols = taps * Cig;
    // dW[g][co][(tap,ci)] = sum_m dY[m][g*Cog + co] * im2col(X)[m][(tap,ci)]
    PlainOp A;  // rows = m (reduction), cols = co
    A.p = dy; A.ld = g->Cout; A.rows = Mred; A.cols = Cog; A.s_outer = 0; A.s_inner = Cog; A.inner = g->groups;
    A.vec = (aligned16(dy) && g->Cout % 4 == 0 && Cog % 4 == 0) ? 1 : 0;
    Im2colOp Bx;  // rows = m, cols = (tap, ci)
    Bx.x = x; Bx.Hi = g->Hi; Bx.Wi = g->Wi; Bx.Ct = g->Cin; Bx.Ho = g->Ho; Bx.Wo = g->Wo; Bx.ks = g->ksize; Bx.stride = g->stride;
    Bx.pad = g->pad; Bx.Cg = Cig; Bx.rows = Mred; Bx.cols = Ncols; Bx.coff = 0;
    Bx.vec = (aligned16(x) && Cig % 4 == 0 && g->Cin % 4 == 0) ? 1 : 0;
    const bool swapped = wgrad_swapped(g, accumulate);
    const GemmEpi ep = wgrad_epi(g, dw, accumulate, ws, ws_floats, swapped);
    if (swapped) return launch_gemm<Im2colOp, false, PlainOp, false>(Bx, A, ep, Ncols, Cog, Mred, g->groups, true, stream, wgrad_site(true));
    return launch_gemm<PlainOp, false, Im2colOp, false>(A, Bx, ep, Cog, Ncols, Mred, g->groups, true, stream, wgrad_site(false));
}

extern "C" int tf_conv2d_wgrad_f32(const tf_conv_geom* g, const float* dy, const float* x, float* dw, int accumulate, void* stream) {
    return conv2d_wgrad(g, dy, x, dw, accumulate, nullptr, 0, stream);
}
// the same with caller scratch for the ordered slab k-split (tf_set_deterministic); tf_conv2d_wgrad_ws_floats: what the plan of an accumulating call
// of this geometry uses of it
extern "C" int tf_conv2d_wgrad_ws_f32(const tf_conv_geom* g, const float* dy, const float* x, float* dw, int accumulate, float* ws, long ws_floats, void* stream) {
    TF_REQUIRE(ws_floats >= 0 && (!ws || aligned16(ws)), "tf_conv2d_wgrad_ws_f32: ws must be 16-byte aligned");
    return conv2d_wgrad(g, dy, x, dw, accumulate, ws, ws_floats, stream);
}
extern "C" long tf_conv2d_wgrad_ws_floats(const tf_conv_geom* g) {
    if (!g || check_geom(g, "tf_conv2d_wgrad_ws_floats")) return 0;
    const int Cog = g->Cout / g->groups, Ncols = g->ksize * g->ksize * (g->Cin / g->groups), Mred = g->B * g->Ho * g->Wo;
    const bool swapped = wgrad_swapped(g, 1);
    const GemmEpi ep = wgrad_epi(g, nullptr, 1, nullptr, 0, swapped);
    return plan_scratch_floats(plan_call(wgrad_site(swapped), swapped ? Ncols : Cog, swapped ? Cog : Ncols, Mred, g->groups, true, true, false, ep));
}
