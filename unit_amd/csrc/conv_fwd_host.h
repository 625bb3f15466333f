// conv_fwd_host.h -- host side of every forward / dgrad conv launch: THE checks of a layer's geometry and THE fill of the argument blocks'
// shared prefix (conv_core_fill), the defaults of Conv256Args' own fields (conv256_defaults), the divide-magic rule, the position-class gate and
// the second problem of a pair launch (unit_fill_second). Nothing in here launches. A new geometry rule goes into conv_core_fill, a new field of
// Conv256Args is defaulted in conv256_defaults -- and nowhere else; the entries override only what they use.
#pragma once
#include "conv_igemm256.h"

struct UnitConvSecond {          // mirrors include/unit_hip.h
  const void* x; void* y; const void* residual; const void* mask_ref;
  int N, H, W, OHf, OWf;
};

// what differs between the families' checks: the multiples C and ldy must be, and the texts of unit_last_error()
struct ConvRules {
  int c_mult, ldy_mult;
  const char *c_msg, *ldy_msg, *shape_msg, *scatter_msg, *align_msg, *size_msg;
};
// prefix: the family's name in its messages; c_words: how the message spells c_mult; ldy_mult: a literal; size_tail: appended to the 4 GiB message
#define CONV_RULES(prefix, c_mult, c_words, ldy_mult, size_tail)                                                                            \
  ConvRules{c_mult, ldy_mult, prefix ": C must be a multiple of " c_words, prefix ": ldy must be a multiple of " #ldy_mult " and >= K",     \
            prefix ": OH/OW mismatch", prefix ": output scatter out of range", prefix ": 16B alignment",                                    \
            prefix ": operand larger than 4 GiB" size_tail}

// Checks the geometry every entry shares and fills the shared prefix from it (tiles_m / tiles_n belong to the launchers).
// C: channels of x as the caller counts them; Cv: channels the kernels contract over (C; nseg * C virtual channels of bf16x3 operands; C + C2
// with a second input); x_row_bytes: bytes of one pixel row of x; w_esz: bytes per weight element.
inline int conv_core_fill(ConvCore& a, const ConvRules& r, const void* x, const void* w, void* y, const float* bias, const void* residual,
                          const void* mask_ref, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int OH, int OW, int ldy,
                          int oy_mul, int OHf, int OWf, int relu, size_t x_row_bytes, int Cv, size_t w_esz) {
  UNIT_CHECK_ARG(C % r.c_mult == 0, r.c_msg);
  UNIT_CHECK_ARG(ldy % r.ldy_mult == 0 && ldy >= K, r.ldy_msg);
  UNIT_CHECK_ARG(OH == (H + 2 * pad - R) / stride + 1 && OW == (W + 2 * pad - S) / stride + 1, r.shape_msg);
  UNIT_CHECK_ARG((OH - 1) * oy_mul < OHf && (OW - 1) * oy_mul < OWf, r.scatter_msg);
  UNIT_CHECK_ARG(((uintptr_t)x % 16 == 0) && ((uintptr_t)w % 16 == 0) && ((uintptr_t)y % 16 == 0), r.align_msg);
  a.x = x; a.w = w; a.y = y; a.bias = bias; a.residual = residual; a.mask_ref = mask_ref;
  a.N = N; a.H = H; a.W = W; a.C = Cv; a.K = K; a.R = R; a.S = S; a.stride = stride; a.pad = pad;
  a.OH = OH; a.OW = OW; a.ldy = ldy; a.oy_mul = oy_mul; a.OHf = OHf; a.OWf = OWf; a.relu = relu;
  a.Kgemm = R * S * Cv; a.M = N * OH * OW;
  size_t xb = (size_t)N * H * W * x_row_bytes, wb = (size_t)K * R * S * Cv * w_esz;
  UNIT_CHECK_ARG(xb < 0xFFFFFFF0ull && wb < 0xFFFFFFF0ull, r.size_msg);          // 32-bit buffer offsets
  a.x_bytes = (unsigned)xb; a.w_bytes = (unsigned)wb;
  return UNIT_OK;
}

// ceil(2^32 / OW), ceil(2^32 / OH) when every pixel index m of a problem of M pixels satisfies m * max(OW, OH) < 2^32 (fast_div, conv_epilogue.h;
// tiles overhang M by less than 512 rows), else 0: the kernels divide
inline void conv_div_magics(int M, int OH, int OW, unsigned& magic_ow, unsigned& magic_oh) {
  bool ok = (unsigned long long)(M + 512) * (unsigned long long)(OW > OH ? OW : OH) < 0xFFFFFFFFull;
  magic_ow = ok ? div_magic((unsigned)OW) : 0u; magic_oh = ok ? div_magic((unsigned)OH) : 0u;
}

// Conv256Args' own fields for a plain launch of the filled prefix: no extended epilogue, no second input, row-major tiles, no second problem,
// plain bf16 operands
inline void conv256_defaults(Conv256Args& a) {
  a.ex = EpiExtra{nullptr, nullptr, nullptr, 0}; a.ex_on = 0;
  a.x2 = nullptr; a.x2_bytes = 0; a.cb_split = 0; a.ratio2 = 1; a.pm_ncls = 0;
  conv_div_magics(a.M, a.OH, a.OW, a.magic_ow, a.magic_oh);
  a.second.on = 0; a.sk = SplitK{0, 0, 0, 0}; a.mask_pitch = 0;
}

// May a layer run on position-class tiles (Conv256Args::pm_ncls)? A 3x3 s1 p1 "same" conv on a small map with a plain (unscattered) output of
// out_esz bytes per element (2: bf16, 4: split) under 4 GiB
inline bool conv_position_classes_apply(const ConvCore& a, size_t out_esz) {
  return a.R == 3 && a.S == 3 && a.stride == 1 && a.pad == 1 && a.OH == a.H && a.OW == a.W && a.oy_mul == 1 && a.OHf == a.OH && a.OWf == a.OW &&
         a.H * a.W <= 4096 && (size_t)a.N * a.H * a.W * a.ldy * out_esz < 0xFFFFFFF0ull;
}

// ConvSecond of a layer (R, S, stride, pad, scatter multiplier shared with the first problem) from the public descriptor; x_row_bytes as in
// conv_core_fill
inline int unit_fill_second(ConvSecond& s, const UnitConvSecond* u, int R, int S, int stride, int pad, int oy_mul, size_t x_row_bytes) {
  s.on = 0; s.tiles0 = 0;
  if (u == nullptr) return UNIT_OK;
  UNIT_CHECK_ARG(u->x != nullptr && u->y != nullptr && u->N >= 0 && u->H > 0 && u->W > 0, "conv pair: second problem needs x, y and positive sizes");
  UNIT_CHECK_ARG(((uintptr_t)u->x % 16 == 0) && ((uintptr_t)u->y % 16 == 0), "conv pair: 16B alignment");
  s.x = u->x; s.y = u->y; s.residual = u->residual; s.mask_ref = u->mask_ref;
  s.N = u->N; s.H = u->H; s.W = u->W;
  s.OH = (u->H + 2 * pad - R) / stride + 1; s.OW = (u->W + 2 * pad - S) / stride + 1;
  s.OHf = u->OHf; s.OWf = u->OWf;
  UNIT_CHECK_ARG(s.OH > 0 && s.OW > 0 && (s.OH - 1) * oy_mul < s.OHf && (s.OW - 1) * oy_mul < s.OWf, "conv pair: second output scatter out of range");
  s.M = u->N * s.OH * s.OW;
  size_t xb = (size_t)u->N * u->H * u->W * x_row_bytes;
  UNIT_CHECK_ARG(xb < 0xFFFFFFF0ull, "conv pair: operand larger than 4 GiB");
  s.x_bytes = (unsigned)xb;
  conv_div_magics(s.M, s.OH, s.OW, s.magic_ow, s.magic_oh);
  s.tiles_m = 0;
  s.on = s.M > 0 ? 1 : 0;
  return UNIT_OK;
}

// the families' entry points with an optional second problem: the extern "C" functions of include/unit_hip.h are thin wrappers (second == nullptr),
// unit_conv2d_fwd_pair dispatches here
int unit_conv_generic_impl(const void* x, const void* w, void* y, const float* bias, const void* residual, const void* mask_ref, int in_dtype,
                           int out_dtype, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int OH, int OW, int ldy, int oy_mul,
                           int OHf, int OWf, int relu, int tile_cfg, const UnitConvSecond* second, void* stream);
int unit_conv_mid_impl(const void* x, const void* w, void* y, const float* bias, const void* residual, const void* mask_ref, int out_dtype, int N,
                       int H, int W, int C, int K, int R, int S, int stride, int pad, int OH, int OW, int ldy, int oy_mul, int OHf, int OWf, int relu,
                       int tile, const UnitConvSecond* second, void* stream);
int unit_conv_big_impl(const void* x, const void* w, void* y, const float* bias, const void* residual, const void* mask_ref, int out_dtype, int N,
                       int H, int W, int C, int K, int R, int S, int stride, int pad, int OH, int OW, int ldy, int oy_mul, int OHf, int OWf, int relu,
                       int variant, const UnitConvSecond* second, void* stream);
int unit_conv_x3_impl(const void* x, const void* w, void* y, const float* bias, const void* residual, const void* mask_ref, int mask_c, int N, int H,
                      int W, int C, int K, int R, int S, int stride, int pad, int OH, int OW, int ldy, int oy_mul, int OHf, int OWf, int relu, int tile,
                      const UnitConvSecond* second, void* stream, int segs);
