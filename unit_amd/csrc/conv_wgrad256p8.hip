// conv_wgrad256p8.hip -- the 256 (k = (r,s,c)) x 256 (n = out channel) weight-gradient tile of conv_wgrad256.hip with the
// schedule of conv_igemm256p8.hip: every 64-pixel step is cut into FOUR phases of 16 MFMAs (one 64 x 32 quadrant of the
// wave's 128 x 64 tile, both 32-pixel sub-steps), the two operand tiles are cut into FOUR 16 KB half-tiles staged one per
// phase under a counted vmcnt, the two wave groups (waves 0-3 / 4-7) run half a phase apart, and the transposing fragment
// reads of phase p+1 are issued inside the MFMA section of phase p.
//
//   dW[n][k] = sum_m dy[m][n] * im2col(x)[m][k]     (contract, split-M slab layout and epilogue: conv_wgrad256.hip)
//
// LDS (128 KB): buffer d = step & 1, slots [X0 | D0 | D1 | X1], each 64 pixel rows x 256 B (128 columns):
//   X half q holds columns  wkr*128 + q*64 + i  of the 256-column x tile at half-column wkr*64 + i   (wkr = 0,1 ; i < 64)
//   D half q holds columns  wnr*64  + q*32 + j  of the 256-column dy tile at half-column wnr*32 + j  (wnr = 0..3 ; j < 32)
// so wave (wk, wn) still owns the contiguous 128 (k) x 64 (n) block. One LDS-DMA piece = 4 rows x 256 B; the 32-B column
// blocks of a row are XOR-swizzled with (row & 7) on the source side (8 blocks per row: a half-wave of ds_read_b64_tr_b16
// touches 8 rows x 32 B on 8 different bank groups).
// Two loop schedules (template parameter SCHED of the tile; UNIT_WGRAD_LOOP / unit_wgrad256_loop() choose per launch), same barriers, same
// staging order, same MFMA order into every accumulator, same m permutation inside a fragment as conv_wgrad256.hip: bit-identical slabs.
// Step t (d = t & 1), fragments fx / fxb (x quadrant columns) and fd0 / fd1 (dy):
//   phase 0: stage X1(t+1) ; quadrant (0,0) = fx  x fd0        phase 2: stage D0(t+2), vmcnt wait (step t+1 landed) ; (1,0) = fxb x fd0
//   phase 1: stage X0(t+2) ; quadrant (0,1) = fx  x fd1        phase 3: stage D1(t+2) ; (1,1) = fxb x fd1
// SCHED 0 (the first schedule, kept for A/B runs and as the reference of tests/test_wgrad_loop_gpu.py): transposing reads per phase 8 / 16 /
//   0 / 24 -- D1(t) -> fd1 | X1(t) -> fxb | none | X0(t+1) -> fx, D0(t+1) -> fd0 -- handed to sched_group_barrier, every read with an address
//   add of its own, and every staging section looks up its rows' table words and waits for them before it can issue its two DMA pieces.
// SCHED 1 (default; profiles/r07_wgrad_loop.txt): 8 / 16 / 8 / 16 -- D1(t) | X1(t) | X0(t+1) columns 0-1 | X0(t+1) columns 2-3, D0(t+1) --
//   one fragment (two reads) per MFMA gap from the first gap on, every gap closed by a scheduling barrier, addresses = six per-lane bases
//   that move by +-BUF once per step + the read's offset field. X0(t+1) is read one phase earlier than before, so phase 1 waits for this
//   wave's pieces of it (counted vmcnt(8), the oldest of ten in flight): both groups have waited one barrier interval before either reads.
//   The rows' table words are fetched once per step (phase 0's staging section, retired by that phase's lgkmcnt wait) and turned into two byte
//   offsets per operand that the step's four staging sections only add a constant to; pointwise layers walk the same straight-line path.
// WAR / RAW distances are those of conv_igemm256p8.hip (reads retired by lgkmcnt(0) before the barrier that ends their MFMA section; a slot
// is restaged >= 2 phases after its last read; first read of a staged half-tile one phase after both groups' vmcnt wait for it).
#include "conv_wgrad256.h"

#ifndef W8_DEFAULT_SCHED
#define W8_DEFAULT_SCHED 1
#endif

#ifdef UNIT_W8_STAMP
// diagnostic build (tools/w8_stamp.sh): waves 0 and 4 (one per wave group) of every 29th workgroup stamp s_memtime in the middle step of their
// loop -- [0] top of the step, [1 + i] behind the step's i-th barrier (staging section, MFMA section, ... of phases 0-3) -- and at [9] loop
// entry, [10] loop exit, [11] tile entry, [12] slab stores issued; [13] = steps, [14] = blockIdx.x, [15] = wave. Kept in scalar registers
// (low 32 bits: only differences are read) until the slab is out -- a store inside the loop would join the counted vmcnt queue -- then written
// by lane 0 with plain vector stores.
__device__ unsigned long long g_w8_stamp[64 * 16];
extern "C" int unit_debug_read_w8_stamps(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_w8_stamp), sizeof(unsigned long long) * 64 * 16, 0, hipMemcpyDeviceToHost);
}
#define W8_STAMP_INIT()                                                                                   \
  unsigned ts[13];                                                                                        \
  _Pragma("unroll") for (int i = 0; i < 13; ++i) ts[i] = 0;                                               \
  const bool stamp_on = (wid & 3) == 0 && blockIdx.x % 29 == 0 && blockIdx.x / 29 < 32;                   \
  const int stamp_t = nsteps >> 1;                                                                        \
  if (stamp_on) ts[11] = (unsigned)__builtin_amdgcn_s_memtime()
#define W8_STAMP(i) do { if (stamp_on) ts[(i)] = (unsigned)__builtin_amdgcn_s_memtime(); } while (0)
#define W8_STAMP_T(i) do { if (stamp_on && t == stamp_t) ts[(i)] = (unsigned)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define W8_STAMP_INIT() do { } while (0)
#define W8_STAMP(i) do { } while (0)
#define W8_STAMP_T(i) do { } while (0)
#endif

// ds_read_b64_tr_b16 with the slot / sub-step / half of the address as the instruction's offset field (conv_wgrad256.h: ds_tr16 -- the same
// rules apply to its result), so that a fragment read needs no address arithmetic of its own between the MFMAs
template <int OFF>
__device__ __forceinline__ s16x4 ds_tr16_o(unsigned a) {
  static_assert(OFF >= 0 && OFF < 65536, "16-bit offset field");
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(a), "i"(OFF) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ bf16x8 tr_frag_o(unsigned a) {
  s16x4 lo = ds_tr16_o<OFF>(a);
  s16x4 hi = ds_tr16_o<OFF + 4096>(a);
  s16x8_w v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// one 256 x 256 tile of dW over the pixels [split * mps, +mps) of a contraction of Meff rows. vo (Wgrad256Args::valid_only): the rows are
// (image, valid output position of the tile's filter tap): positions = rows v_oh0.. of the map, columns v_ow0.. of v_cw, nv per image.
// TABN: entries of the pixel -> input offset table behind the operand stages (maps of up to TABN pixels avoid per-row divisions).
template <int TABN, int SCHED>
__device__ __forceinline__ void wgrad256_p8_tile(const Wgrad256Args& p, int tile_k, int tile_n, int split, const bool vo, int v_oh0, int v_ow0,
                                                 int v_cw, int nv, int Meff, int mps, char* smem) {
  constexpr int MS = 64;
  constexpr int HALF = MS * 256;               // 16 KB
  constexpr bool BAL = SCHED == 1, HOIST = SCHED == 1;      // SCHED 1 = reads placed gap by gap (BAL) + staging offsets once per step (HOIST)
  constexpr int SX0 = 0, SD0 = HALF, SD1 = 2 * HALF, SX1 = 3 * HALF, BUF = 4 * HALF;
  if constexpr (BAL) {          // wave-uniform by construction; said so, they stay out of the VGPRs the loop needs
    tile_k = __builtin_amdgcn_readfirstlane(tile_k); tile_n = __builtin_amdgcn_readfirstlane(tile_n); split = __builtin_amdgcn_readfirstlane(split);
  }
  int k0 = tile_k * 256, n0 = tile_n * 256;
  int rs = k0 / p.C, ch0 = k0 - rs * p.C, kr = rs / p.S, ksx = rs - kr * p.S;
  int m_begin = min(Meff, split * mps), m_end = min(Meff, m_begin + mps);

  const bf16_t* __restrict__ X = (const bf16_t*)p.x;
  const bf16_t* __restrict__ DY = (const bf16_t*)p.dy;
  __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(X), 0, (int)p.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(DY), 0, (int)p.dy_bytes, 0x00020000);
  constexpr unsigned OOB = 0xFFFFFFF0u;

  int tid = threadIdx.x, lane = tid & 63;
  int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int wk = wid >> 2, wn = wid & 3;
  const int grp = wk;
  const bool pointwise = (p.R == 1 && p.S == 1 && p.stride == 1 && p.pad == 0);

  // staging: piece j (0,1) of this wave in every half-tile = rows (j*8 + wid)*4 .. +4 ; lane -> row + (lane>>4), physical
  // 16-B chunk lane&15 ; logical chunk = (32-B block XOR (row & 7), 16-B half kept). (row & 7) does not depend on j.
  int s_row[2]; unsigned xcol[2], dcol[2];
  {
    int r0 = wid * 4 + (lane >> 4);
    s_row[0] = r0; s_row[1] = 32 + r0;
    int jp = lane & 15;
    int hcol = ((((jp >> 1) ^ (r0 & 7)) << 1) | (jp & 1)) * 8;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      xcol[q] = (unsigned)(ch0 + (hcol >> 6) * 128 + q * 64 + (hcol & 63));
      dcol[q] = (unsigned)(n0 + (hcol >> 5) * 64 + q * 32 + (hcol & 31));
    }
  }
  // im2col rows without per-step divisions: the (n, pixel-in-image) pair of each of this lane's two piece rows is carried
  // incrementally (+64 pixels per step) and a small LDS table maps the pixel to its input offset for THIS workgroup's filter
  // tap ((ih*W + iw)*C, or -1 outside the map). Table after the operand stages (OHW <= 1024 entries; larger maps divide).
  int* tab = reinterpret_cast<int*>(smem + 2 * BUF);
  int* tabd = tab + 512;                          // valid_only: position index -> output pixel of the dy row (OHW <= 512 then)
  // HOIST: a pointwise layer walks the same path as a table layer -- a "map" of ONE pixel per image (image index = pixel row m, table = {0},
  // image pitch = the row pitch) -- so that the per-step offset arithmetic below has no mode branches
  if constexpr (HOIST) { if (pointwise) { nv = 1; v_cw = 1; v_oh0 = 0; v_ow0 = 0; } }
  const bool use_tab = HOIST ? (pointwise || p.OHW <= TABN) : (!pointwise && p.OHW <= TABN);
  const unsigned img_pitch = pointwise ? (unsigned)p.x_pitch : (unsigned)(p.H * p.W * p.x_pitch);
  int xn[2] = {0, 0}, xp[2] = {0, 0};
  const int adv_q = MS / nv, adv_r = MS - adv_q * nv;
  if (use_tab) {
    for (int px = tid; px < nv; px += 512) {
      int oh = px / v_cw, ow = px - oh * v_cw;
      oh += v_oh0; ow += v_ow0;
      int ih = oh * p.stride - p.pad + kr, iw = ow * p.stride - p.pad + ksx;
      tab[px] = ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) ? (ih * p.W + iw) * p.x_pitch : -1;
      if (vo) tabd[px] = oh * p.OW + ow;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned um = (unsigned)(m_begin + s_row[j]);
      unsigned n = um / (unsigned)nv;
      xn[j] = (int)n; xp[j] = (int)(um - n * (unsigned)nv);
    }
    __syncthreads();
  }
  // (SCHED 1: the divisors of the rows-by-division path are made opaque where they are used, so that hipcc does not keep their reciprocals in
  //  VGPRs across the loop for a path that only problems of 2^32 and more (pixels x map size) take)
  auto opq = [&](int v) { asm volatile("" : "+s"(v)); return v; };
  auto x_advance = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      xn[j] += adv_q; xp[j] += adv_r;
      if (xp[j] >= nv) { xp[j] -= nv; xn[j] += 1; }
    }
  };
  auto stage_x = [&](int q, int d, int mstep) {
    char* base = smem + d * BUF + (q ? SX1 : SX0);
    int tv[2] = {0, 0};
    if (use_tab) {
      // (asm: a plain LDS load here would make hipcc drain vmcnt in front of it, conv_wgrad256.h)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)(tab + xp[j]);
        asm volatile("ds_read_b32 %0, %1" : "=v"(tv[j]) : "v"(a) : "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tv[0]), "+v"(tv[1]) :: "memory");
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int m = mstep + s_row[j];
      bool ok = m < m_end;
      unsigned xoff;
      if (pointwise) xoff = ((unsigned)m * (unsigned)p.x_pitch + xcol[q]) * 2u;
      else if (use_tab) {
        ok = ok && tv[j] >= 0;
        xoff = ((unsigned)xn[j] * (unsigned)(p.H * p.W * p.x_pitch) + (unsigned)tv[j] + xcol[q]) * 2u;
      } else {
        unsigned um = (unsigned)m, n, oh, ow;
        if (p.use_magic) {
          n = __umulhi(um, p.magic_ohw); unsigned rem = um - n * (unsigned)p.OHW;
          if (rem >= (unsigned)p.OHW) { rem -= p.OHW; ++n; }
          oh = __umulhi(rem, p.magic_ow); ow = rem - oh * (unsigned)p.OW;
          if (ow >= (unsigned)p.OW) { ow -= p.OW; ++oh; }
        } else {
          ow = um % (unsigned)p.OW; unsigned t2 = um / (unsigned)p.OW; oh = t2 % (unsigned)p.OH; n = t2 / (unsigned)p.OH;
        }
        int ih = (int)oh * p.stride - p.pad + kr, iw = (int)ow * p.stride - p.pad + ksx;
        ok = ok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        xoff = ((unsigned)n * (unsigned)(p.H * p.W * p.x_pitch) + (unsigned)((ih * p.W + iw) * p.x_pitch) + xcol[q]) * 2u;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, (lds_void_w*)(base + (j * 8 + wid) * 1024), 16, ok ? xoff : OOB, 0, 0, 0);
    }
  };
  auto stage_d = [&](int q, int d, int mstep) {
    char* base = smem + d * BUF + (q ? SD1 : SD0);
    int tv[2] = {0, 0};
    if (vo) {                                     // the dy row of (image xn, valid position xp): table lookup, as stage_x
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)(tabd + xp[j]);
        asm volatile("ds_read_b32 %0, %1" : "=v"(tv[j]) : "v"(a) : "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tv[0]), "+v"(tv[1]) :: "memory");
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int m = mstep + s_row[j];
      unsigned doff = ((unsigned)(vo ? xn[j] * p.OHW + tv[j] : m) * (unsigned)p.ldy + dcol[q]) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsD, (lds_void_w*)(base + (j * 8 + wid) * 1024), 16, m < m_end ? doff : OOB, 0, 0, 0);
    }
  };

  // HOIST: the four half-tiles of a step stage the same pixel rows, so their table words are fetched ONCE per step -- issued in the
  // staging section of phase 0, retired by the lgkmcnt wait that ends that phase's MFMA section -- and turned into the byte offsets of
  // half 0 (xo / dof, OOB for a row outside the split or the map) that the step's four staging sections only add a constant to.
  unsigned xo[2] = {OOB, OOB}, dof[2] = {OOB, OOB};
  int tvx[2] = {0, 0}, tvd[2] = {0, 0};
  const int tabd_off = vo ? 512 : 0;
  auto lookup = [&]() {
    if (use_tab) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)(tab + xp[j]);
        asm volatile("ds_read_b32 %0, %1" : "=v"(tvx[j]) : "v"(a) : "memory");
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {          // (not valid_only: the x word again, unused)
        unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)(tab + tabd_off + xp[j]);
        asm volatile("ds_read_b32 %0, %1" : "=v"(tvd[j]) : "v"(a) : "memory");
      }
    }
  };
  auto lookup_wait = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tvx[0]), "+v"(tvx[1]), "+v"(tvd[0]), "+v"(tvd[1]) :: "memory"); };
  const unsigned vo_mask = vo ? ~0u : 0u;
  auto prep = [&](int mstep) {
    // straight-line for table layers (pointwise included); only maps wider than the table branch, into the division path
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int m = mstep + s_row[j];
      bool ok = m < m_end;
      unsigned xoff = ((unsigned)xn[j] * img_pitch + (unsigned)tvx[j] + xcol[0]) * 2u;
      xo[j] = (ok && tvx[j] >= 0) ? xoff : OOB;
      unsigned drow = (((unsigned)(xn[j] * p.OHW + tvd[j])) & vo_mask) | ((unsigned)m & ~vo_mask);
      dof[j] = ok ? (drow * (unsigned)p.ldy + dcol[0]) * 2u : OOB;
    }
    if (!use_tab) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int m = mstep + s_row[j];
        unsigned um = (unsigned)m, n, oh, ow;
        if (p.use_magic) {
          n = __umulhi(um, p.magic_ohw); unsigned rem = um - n * (unsigned)p.OHW;
          if (rem >= (unsigned)p.OHW) { rem -= p.OHW; ++n; }
          oh = __umulhi(rem, p.magic_ow); ow = rem - oh * (unsigned)p.OW;
          if (ow >= (unsigned)p.OW) { ow -= p.OW; ++oh; }
        } else {
          const unsigned dow = (unsigned)opq(p.OW), doh = (unsigned)opq(p.OH);
          ow = um % dow; unsigned t2 = um / dow; oh = t2 % doh; n = t2 / doh;
        }
        int ih = (int)oh * p.stride - p.pad + kr, iw = (int)ow * p.stride - p.pad + ksx;
        bool okx = m < m_end && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        unsigned xoff = ((unsigned)n * (unsigned)(p.H * p.W * p.x_pitch) + (unsigned)((ih * p.W + iw) * p.x_pitch) + xcol[0]) * 2u;
        xo[j] = okx ? xoff : OOB;
      }
    }
  };
  // (half 1 = half 0 + 64 columns of x / + 32 columns of dy: xcol / dcol above)
  auto stage_xh = [&](int q, int d) {
    char* base = smem + d * BUF + (q ? SX1 : SX0);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, (lds_void_w*)(base + (j * 8 + wid) * 1024), 16, xo[j] == OOB ? OOB : xo[j] + (unsigned)(q * 128), 0, 0, 0);
  };
  auto stage_dh = [&](int q, int d) {
    char* base = smem + d * BUF + (q ? SD1 : SD0);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsD, (lds_void_w*)(base + (j * 8 + wid) * 1024), 16, dof[j] == OOB ? OOB : dof[j] + (unsigned)(q * 64), 0, 0, 0);
  };
#define W8_STAGE_X(Q, D, M) do { if constexpr (HOIST) stage_xh(Q, D); else stage_x(Q, D, M); } while (0)
#define W8_STAGE_D(Q, D, M) do { if constexpr (HOIST) stage_dh(Q, D); else stage_d(Q, D, M); } while (0)

  f32x4 acc[8][4];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment addressing (tr_frag of conv_wgrad256.hip on 256-B rows): lane l: g = l>>4, i = l&15 = 4q+pq reads rows
  // 32*sub + 16h + 4g + q, 8 B at column block (col>>4) ^ (row & 7); element j = 4h+q' of lane i <-> m-row 32*sub+16h+4g+q'
  int offx[4], offd[2];
  {
    int g = lane >> 4, i = lane & 15, q4 = i >> 2, pq = i & 3;
    int rowl = 4 * g + q4, r7 = rowl & 7;
    int basel = rowl * 256 + 8 * pq;
#pragma unroll
    for (int a = 0; a < 4; ++a) offx[a] = basel + (((wk * 4 + a) ^ r7) << 5);
#pragma unroll
    for (int b = 0; b < 2; ++b) offd[b] = basel + (((wn * 2 + b) ^ r7) << 5);
  }
  auto frag = [&](const char* half, int off, int sub) -> bf16x8 {
    const char* a0 = half + off + sub * 8192;
    s16x4 lo = ds_tr16(a0);
    s16x4 hi = ds_tr16(a0 + 4096);
    s16x8_w v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  bf16x8 fx[4][2], fxb[4][2], fd0[2][2], fd1[2][2];
  // BAL: per-lane LDS addresses of the fragment rows in the buffer being read (cx: x column blocks, cd: dy); a step reads buffer d in phases
  // 0-1 and buffer d ^ 1 in phases 2-3, so they move by +-BUF once per step and everything else is the offset field of the read
  unsigned cx[4], cd[2];
  {
    unsigned sb = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)smem;
#pragma unroll
    for (int a = 0; a < 4; ++a) cx[a] = sb + (unsigned)offx[a];
#pragma unroll
    for (int b = 0; b < 2; ++b) cd[b] = sb + (unsigned)offd[b];
  }
#define W8_UX(FX, A, SUB, SLOT) FX[A][SUB] = tr_frag_o<(SLOT) + (SUB) * 8192>(cx[A])
#define W8_UD(FD, B, SUB, SLOT) FD[B][SUB] = tr_frag_o<(SLOT) + (SUB) * 8192>(cd[B])
#define W8_FX(FX, A, SLOT) do { W8_UX(FX, A, 0, SLOT); W8_UX(FX, A, 1, SLOT); } while (0)
#define W8_FD(FD, B, SLOT) do { W8_UD(FD, B, 0, SLOT); W8_UD(FD, B, 1, SLOT); } while (0)
#define W8_READ_X(HALFP, FX)                                                          \
  do {                                                                                \
    _Pragma("unroll") for (int a = 0; a < 4; ++a)                                     \
      _Pragma("unroll") for (int sub = 0; sub < 2; ++sub) FX[a][sub] = frag(HALFP, offx[a], sub); \
  } while (0)
#define W8_READ_D(HALFP, FD)                                                          \
  do {                                                                                \
    _Pragma("unroll") for (int b = 0; b < 2; ++b)                                     \
      _Pragma("unroll") for (int sub = 0; sub < 2; ++sub) FD[b][sub] = frag(HALFP, offd[b], sub); \
  } while (0)
#define W8_BAR() do { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); } while (0)
#if defined(UNIT_DBGW8) && (UNIT_DBGW8 & 4)
#define W8_FMA(ACC, A, B) do { if (b == 0) ACC += __builtin_bit_cast(f32x4, A); if (a == 0) ACC += __builtin_bit_cast(f32x4, B); } while (0)
#else
#define W8_FMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, ACC, 0, 0, 0)
#endif
#if defined(UNIT_DBGW8) && (UNIT_DBGW8 & 8)
#define W8_RD(stmt) do { if (t == 0) { stmt; } } while (0)
#else
#define W8_RD(stmt) do { stmt; } while (0)
#endif
  // MFMA section: quadrant (QX, QN) = acc[QX*4 ..][QN*2 ..]; NR ds_read_b64_tr_b16 of READS spread PER per MFMA gap
#define W8_MM(QX, QN, FX, FD, NR, PER, READS)                                          \
  do {                                                                                 \
    __builtin_amdgcn_s_setprio(1);                                                     \
    READS;                                                                             \
    _Pragma("unroll") for (int sub = 0; sub < 2; ++sub)                                \
      _Pragma("unroll") for (int a = 0; a < 4; ++a)                                    \
        _Pragma("unroll") for (int b = 0; b < 2; ++b)                                  \
          W8_FMA(acc[(QX) * 4 + a][(QN) * 2 + b], FX[a][sub], FD[b][sub]);             \
    _Pragma("unroll") for (int i = 0; i < (NR) / ((PER) > 0 ? (PER) : 1); ++i) {      \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                               \
      __builtin_amdgcn_sched_group_barrier(0x100, (PER), 0);                           \
    }                                                                                  \
    __builtin_amdgcn_sched_group_barrier(0x008, 16 - (NR) / ((PER) > 0 ? (PER) : 1), 0); \
    __builtin_amdgcn_s_setprio(0);                                                     \
    if ((NR) > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                   \
  } while (0)

  // BAL: the section written out gap by gap. sched_group_barrier does not place the asm reads (in the SCHED 0 code object they sit in clumps,
  // nine of them in front of the first MFMA of phase 3, one behind the last MFMA of phase 1), so here every gap is closed by a scheduling
  // barrier: gap i = the reads R<i> (one fragment = two ds_read_b64_tr_b16, or none), then MFMA i -- same MFMA order as W8_MM. The reads
  // sit in the first gaps, the MFMAs behind them run over their latency, and the section ends with the same lgkmcnt(0).
#define W8_GAP(QX, QN, FX, FD, I, READS)                                               \
  do {                                                                                 \
    W8_RD(READS);                                                                      \
    { constexpr int sub = (I) >> 3, a = ((I) >> 1) & 3, b = (I) & 1;                   \
      W8_FMA(acc[(QX) * 4 + a][(QN) * 2 + b], FX[a][sub], FD[b][sub]); }               \
    __builtin_amdgcn_sched_barrier(0);                                                 \
  } while (0)
#define W8_MMX(QX, QN, FX, FD, R0, R1, R2, R3, R4, R5, R6, R7)                         \
  do {                                                                                 \
    __builtin_amdgcn_s_setprio(1);                                                     \
    W8_GAP(QX, QN, FX, FD, 0, R0); W8_GAP(QX, QN, FX, FD, 1, R1); W8_GAP(QX, QN, FX, FD, 2, R2); W8_GAP(QX, QN, FX, FD, 3, R3); \
    W8_GAP(QX, QN, FX, FD, 4, R4); W8_GAP(QX, QN, FX, FD, 5, R5); W8_GAP(QX, QN, FX, FD, 6, R6); W8_GAP(QX, QN, FX, FD, 7, R7); \
    W8_GAP(QX, QN, FX, FD, 8, (void)0); W8_GAP(QX, QN, FX, FD, 9, (void)0); W8_GAP(QX, QN, FX, FD, 10, (void)0); W8_GAP(QX, QN, FX, FD, 11, (void)0); \
    W8_GAP(QX, QN, FX, FD, 12, (void)0); W8_GAP(QX, QN, FX, FD, 13, (void)0); W8_GAP(QX, QN, FX, FD, 14, (void)0); W8_GAP(QX, QN, FX, FD, 15, (void)0); \
    __builtin_amdgcn_s_setprio(0);                                                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                 \
  } while (0)
#define W8_NR (void)0

  constexpr int PER0 = 1, PER1 = 1, PER3 = 2;          // SCHED 0: transposing fragment reads per MFMA gap in phases 0 / 1 / 3
  const int nsteps = (m_end - m_begin + MS - 1) / MS;
  W8_STAMP_INIT();
  if (nsteps > 0) {
    int mst = m_begin;
    if constexpr (HOIST) { lookup(); lookup_wait(); prep(mst); }
    W8_STAGE_X(0, 0, mst); W8_STAGE_D(0, 0, mst); W8_STAGE_D(1, 0, mst); W8_STAGE_X(1, 0, mst);
    mst += MS; x_advance();
    if (nsteps > 1) {
      if constexpr (HOIST) { lookup(); lookup_wait(); prep(mst); }
      W8_STAGE_X(0, 1, mst); W8_STAGE_D(0, 1, mst); W8_STAGE_D(1, 1, mst);
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    W8_BAR();
    if constexpr (BAL) {
      W8_FD(fd0, 0, SD0); W8_FD(fd0, 1, SD0);
      W8_FX(fx, 0, SX0); W8_FX(fx, 1, SX0); W8_FX(fx, 2, SX0); W8_FX(fx, 3, SX0);
    } else {
      W8_READ_D(smem + SD0, fd0);
      W8_READ_X(smem + SX0, fx);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (grp == 1) W8_BAR();
    W8_STAMP(9);
    for (int t = 0; t < nsteps; ++t) {
      const int d = t & 1;
      const char* buf = smem + d * BUF;
      const char* bnx = smem + (d ^ 1) * BUF;
#if defined(UNIT_DBGW8) && (UNIT_DBGW8 & 2)
      const bool n1 = false, n2 = false;
#else
      const bool n1 = t + 1 < nsteps, n2 = t + 2 < nsteps;
#endif
      W8_STAMP_T(0);
      // phase 0
      if (n1) W8_STAGE_X(1, d ^ 1, mst);
      mst += MS; x_advance();
      if constexpr (HOIST) lookup();                     // step t+2's table words (xp stays inside the table past the last step)
      W8_BAR(); W8_STAMP_T(1);
      if constexpr (BAL) W8_MMX(0, 0, fx, fd0, W8_UD(fd1, 0, 0, SD1), W8_UD(fd1, 1, 0, SD1), W8_UD(fd1, 0, 1, SD1), W8_UD(fd1, 1, 1, SD1), W8_NR, W8_NR, W8_NR, W8_NR);
      else W8_MM(0, 0, fx, fd0, 8, PER0, W8_RD(W8_READ_D(buf + SD1, fd1)));
      if constexpr (HOIST) lookup_wait();
      W8_BAR(); W8_STAMP_T(2);
      // phase 1 (BAL: X0(t+1) is read from phase 2 on, so this wave's pieces of it -- the oldest of the ten in flight -- have to land here)
      if (n2) {
        if constexpr (HOIST) prep(mst);
        W8_STAGE_X(0, d, mst);
        if constexpr (BAL) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else if (BAL && n1) {
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      }
      W8_BAR(); W8_STAMP_T(3);
      if constexpr (BAL) W8_MMX(0, 1, fx, fd1, W8_UX(fxb, 0, 0, SX1), W8_UX(fxb, 1, 0, SX1), W8_UX(fxb, 2, 0, SX1), W8_UX(fxb, 3, 0, SX1), W8_UX(fxb, 0, 1, SX1), W8_UX(fxb, 1, 1, SX1), W8_UX(fxb, 2, 1, SX1), W8_UX(fxb, 3, 1, SX1));
      else W8_MM(0, 1, fx, fd1, 16, PER1, W8_RD(W8_READ_X(buf + SX1, fxb)));
      W8_BAR(); W8_STAMP_T(4);
      // phase 2
      if constexpr (BAL) {                               // the fragment addresses move to the other buffer: step t+1's
        const unsigned flip = d ? (unsigned)-BUF : (unsigned)BUF;
#pragma unroll
        for (int a = 0; a < 4; ++a) cx[a] += flip;
#pragma unroll
        for (int b = 0; b < 2; ++b) cd[b] += flip;
      }
      if (n2) {
        W8_STAGE_D(0, d, mst);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      W8_BAR(); W8_STAMP_T(5);
      if constexpr (BAL) W8_MMX(1, 0, fxb, fd0, W8_UX(fx, 0, 0, SX0), W8_UX(fx, 1, 0, SX0), W8_UX(fx, 0, 1, SX0), W8_UX(fx, 1, 1, SX0), W8_NR, W8_NR, W8_NR, W8_NR);
      else W8_MM(1, 0, fxb, fd0, 0, 0, (void)0);
      W8_BAR(); W8_STAMP_T(6);
      // phase 3 (after the last step the reads fetch stale, in-bounds LDS that nobody uses)
      if (n2) W8_STAGE_D(1, d, mst);
      W8_BAR(); W8_STAMP_T(7);
      if constexpr (BAL) W8_MMX(1, 1, fxb, fd1, W8_UX(fx, 2, 0, SX0), W8_UX(fx, 3, 0, SX0), W8_UD(fd0, 0, 0, SD0), W8_UD(fd0, 1, 0, SD0), W8_UX(fx, 2, 1, SX0), W8_UX(fx, 3, 1, SX0), W8_UD(fd0, 0, 1, SD0), W8_UD(fd0, 1, 1, SD0));
      else W8_MM(1, 1, fxb, fd1, 24, PER3, W8_RD(W8_READ_D(bnx + SD0, fd0); W8_READ_X(bnx + SX0, fx)));
      W8_BAR(); W8_STAMP_T(8);
    }
    W8_STAMP(10);
    if (grp == 0) W8_BAR();
  }
#undef W8_MM
#undef W8_MMX
#undef W8_GAP
#undef W8_NR
#undef W8_FMA
#undef W8_RD
#undef W8_BAR
#undef W8_READ_D
#undef W8_READ_X
#undef W8_FX
#undef W8_FD
#undef W8_UX
#undef W8_UD
#undef W8_STAGE_X
#undef W8_STAGE_D

  // epilogue: D[row = k][col = n] -> partial[split][n][k..k+3]
  float* out = p.partial + (size_t)split * p.K * p.Kgemm;
  // (the lane id is taken afresh: nothing the epilogue addresses are made of has to stay in a VGPR across the loop)
  const int elane = BAL ? (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) : lane;
  int fq = elane >> 4, fr = elane & 15;
#if defined(UNIT_DBGW8) && (UNIT_DBGW8 & 1)
  // diagnostic build only (tools/exp_w8.sh): one store per lane instead of 32 -- what does the slab store cost?
  f32x4 ssum = acc[0][0];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int a = 0; a < 8; ++a) if (a + b) ssum += acc[a][b];
  *reinterpret_cast<f32x4*>(out + (size_t)(n0 + wn * 64 + fr) * p.Kgemm + k0 + wk * 128 + fq * 4) = ssum;
#else
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    int n = n0 + wn * 64 + b * 16 + fr;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      int k = k0 + wk * 128 + a * 16 + fq * 4;
      *reinterpret_cast<f32x4*>(out + (size_t)n * p.Kgemm + k) = acc[a][b];
    }
  }
#endif
#ifdef UNIT_W8_STAMP
  W8_STAMP(12);
  if (stamp_on && lane == 0) {
    unsigned long long* g = g_w8_stamp + ((blockIdx.x / 29) * 2 + (wid >> 2)) * 16;
#pragma unroll
    for (int i = 0; i < 13; ++i) g[i] = ts[i];
    g[13] = (unsigned long long)nsteps; g[14] = blockIdx.x; g[15] = (unsigned long long)wid;
  }
#endif
}


template <int SCHED>
__global__ void __launch_bounds__(512, 2) conv_wgrad256_p8_kernel(Wgrad256Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // XCD-aware remap (workgroup b runs on XCD b % 8): every XCD gets a contiguous chunk of (split, tile_n, tile_k) ids, i.e.
  // the tiles of one or two split-M slabs. They walk the same pixel rows at the same pace, so an x / dy row block is
  // fetched from HBM once per XCD and then served to the other tiles of the slab out of that XCD's 4 MB L2.
  int bid = blockIdx.x;
  const bool vo = p.valid_only != 0;
  int tile_k, tile_n, split;
  // valid_only (Wgrad256Args): the contraction index of a tile runs over (image, valid output position of ITS filter tap) instead of
  // all pixels; valid positions = rows v_oh0 .. of the map, columns v_ow0 .. of v_cw (nv per image). The taps differ in work (36 / 42
  // / 49 positions on 7x7) and the grid is one round of workgroups, so with the same split count for every tap the centre tap would
  // set the time: the p.splits slabs include one spare, and 9 * (p.splits - 1) workgroup slots per (channel block, n tile) are dealt to
  // the taps in proportion to their positions (7 x 7, 8 slabs: corners 6, edges 7, centre 8 splits -> 6.0 / 6.0 / 6.1 positions per
  // split instead of 49 / 7). A workgroup past its tap's count ("filler") only leaves its slab tile zero.
  int v_oh0 = 0, v_ow0 = 0, v_cw = p.OW, nv = p.OHW, Meff = p.M, mps = p.m_per_split;
  if (!vo) {
    int nwg = gridDim.x, q = nwg / 8, r = nwg % 8, xcd = bid % 8, loc = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    tile_k = bid % p.tiles_k; int tt = bid / p.tiles_k;
    tile_n = tt % p.tiles_n; split = tt / p.tiles_n;
  } else {
    const int ntap = p.R * p.S, ncb = p.tiles_k / ntap;
    int nh[3], nw[3], sum_h = 0, sum_w = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      nh[t] = max(0, min(p.OH - 1, p.H - 1 + p.pad - t) - max(0, p.pad - t) + 1);
      nw[t] = max(0, min(p.OW - 1, p.W - 1 + p.pad - t) - max(0, p.pad - t) + 1);
      sum_h += nh[t]; sum_w += nw[t];
    }
    const int tot = sum_h * sum_w, slots = ntap * max(1, p.splits - 1);
    int stt[9], sum_st = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      int v = nh[t / 3] * nw[t % 3];
      stt[t] = max(1, min(p.splits, (slots * v + tot / 2) / tot));
      sum_st += stt[t];
    }
    // id map: real work first on every XCD (workgroup b runs on XCD b % 8 and the XCD's workgroups start in id order), fillers last;
    // real items ordered split-major (split j of every tap that has one, all n tiles and channel blocks: they walk about the same
    // pixel rows at the same pace -- shared through the XCD's L2), each XCD a contiguous run of them
    const int per = p.tiles_n * ncb;
    const int RI = per * sum_st, nwg = gridDim.x;
    const int xcd = bid % 8, loc = bid / 8;
    const int start_r = xcd * (RI / 8) + min(xcd, RI % 8), real_x = RI / 8 + (xcd < RI % 8 ? 1 : 0);
    const int start_t = xcd * (nwg / 8) + min(xcd, nwg % 8);
    int tap = 0, cb = 0;
    if (loc < real_x) {
      int L = start_r + loc, j = 0;
      for (;; ++j) {
        int act = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) act += stt[t] > j ? 1 : 0;
        if (L < per * act) {
          tile_n = L / (ncb * act); int rem = L - tile_n * (ncb * act);
          int a = rem / ncb; cb = rem - a * ncb;
#pragma unroll
          for (int t = 8; t >= 0; --t) { int before = 0; for (int u = 0; u < t; ++u) before += stt[u] > j ? 1 : 0; if (stt[t] > j && before == a) tap = t; }
          break;
        }
        L -= per * act;
      }
      split = j;
    } else {
      int z = (start_t - start_r) + (loc - real_x);
      tile_n = 0; split = p.splits;             // (overwritten below; z always lands in a tap)
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        int cnt = (p.splits - stt[t]) * per;
        if (z >= 0 && z < cnt) {
          int jj = z / per, rem = z - jj * per;
          split = stt[t] + jj; tile_n = rem / ncb; cb = rem - tile_n * ncb; tap = t;
          z = -1;
        } else if (z >= 0) z -= cnt;
      }
    }
    tile_k = tap * ncb + cb;
    int kr_ = tap / p.S, ks_ = tap - kr_ * p.S;
    v_oh0 = max(0, p.pad - kr_); v_ow0 = max(0, p.pad - ks_);
    v_cw = nw[ks_]; nv = nh[kr_] * v_cw;
    Meff = p.N * nv;
    int st = stt[tap];
    mps = ((Meff + st - 1) / st + 63) / 64 * 64;
    if (split >= st) Meff = 0;
  }
  wgrad256_p8_tile<1024, SCHED>(p, tile_k, tile_n, split, vo, v_oh0, v_ow0, v_cw, nv, Meff, mps, smem);
}

// which loop schedule a launch runs (the template parameter SCHED of the tile): UNIT_WGRAD_LOOP, read per launch like UNIT_WGRAD_GANG
// (conv_wgrad_plan.hip) so that the tests and A/B runs switch it in-process. Every schedule writes the same slabs bit for bit.
static int wgrad256_loop_sched() {
  const char* e = getenv("UNIT_WGRAD_LOOP");
  int v = e && *e ? atoi(e) : W8_DEFAULT_SCHED;
  return v < 0 || v > 1 ? W8_DEFAULT_SCHED : v;
}

extern "C" int unit_wgrad256_loop(void) { return wgrad256_loop_sched(); }

template <int SCHED>
static int wgrad256_p8_launch_t(const Wgrad256Args& a, hipStream_t st) {
  size_t lds = 8 * 64 * 256 + 4096;      // operand stages + the pixel -> input offset table
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)conv_wgrad256_p8_kernel<SCHED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  conv_wgrad256_p8_kernel<SCHED><<<a.tiles_k * a.tiles_n * a.splits, 512, lds, st>>>(a);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

int unit_wgrad256_p8_launch(const Wgrad256Args& a, hipStream_t st) {
  switch (wgrad256_loop_sched()) {
    case 0: return wgrad256_p8_launch_t<0>(a, st);
    default: return wgrad256_p8_launch_t<1>(a, st);
  }
}

// ---- grouped launch (include/unit_hip.h: unit_conv2d_wgrad_group): the 256x256 tiles of SEVERAL layers in one grid. A unit = the tiles of
// one (layer, split) -- for valid_only layers of one (layer, filter tap, split): they contract over the same rows -- dealt to ONE XCD by
// the host (conv_wgrad_plan.hip), longest first. With the layers of a Res5 head in one grid every layer needs 3-4 split-M slabs instead of
// 8-16 (launched alone, 16 tiles have to become 256 workgroups): a quarter of the slab traffic, 200-step loops; the res4 layers of a
// gradient bucket get 256x256 tiles at all (half the operand bytes per flop of the 128x128 ring kernel).
__device__ __forceinline__ int pinw(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ const void* pinw_ptr(const void* q) {
  unsigned long long u = (unsigned long long)(uintptr_t)q;
  unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return (const void*)(uintptr_t)(((unsigned long long)hi << 32) | lo);
}

template <int SCHED>
__global__ void __launch_bounds__(512, 2) conv_wgrad256_group_kernel(WgradGroupArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  int nu = g.t.n_units[xcd];
  if (slot >= (int)g.t.unit_start[xcd][nu]) return;
  int u = 0;
  for (int i = 1; i < nu; ++i)
    if (slot >= (int)g.t.unit_start[xcd][i]) u = i;
  unsigned code = g.t.unit_code[xcd][u];
  const Wgrad256Args& src = g.p[code & 31];     // into SGPRs once (conv_wgrad128r.hip)
  Wgrad256Args p;
  p.x = pinw_ptr(src.x); p.dy = pinw_ptr(src.dy); p.partial = (float*)pinw_ptr(src.partial);
  p.N = pinw(src.N); p.H = pinw(src.H); p.W = pinw(src.W); p.C = pinw(src.C); p.K = pinw(src.K); p.R = pinw(src.R); p.S = pinw(src.S);
  p.stride = pinw(src.stride); p.pad = pinw(src.pad); p.OH = pinw(src.OH); p.OW = pinw(src.OW); p.ldy = pinw(src.ldy);
  p.Kgemm = pinw(src.Kgemm); p.M = pinw(src.M); p.tiles_k = pinw(src.tiles_k); p.tiles_n = pinw(src.tiles_n); p.splits = pinw(src.splits);
  p.m_per_split = pinw(src.m_per_split); p.x_bytes = (unsigned)pinw((int)src.x_bytes); p.dy_bytes = (unsigned)pinw((int)src.dy_bytes);
  p.magic_ohw = (unsigned)pinw((int)src.magic_ohw); p.magic_ow = (unsigned)pinw((int)src.magic_ow); p.OHW = pinw(src.OHW);
  p.use_magic = pinw(src.use_magic); p.valid_only = pinw(src.valid_only); p.x_pitch = pinw(src.x_pitch);
  int t = slot - (int)g.t.unit_start[xcd][u] + (int)g.t.unit_tile0[xcd][u];
  int tap = (int)((code >> 5) & 15), split = (int)(code >> 9);
  if (p.valid_only) {
    int ncb = p.tiles_k / (p.R * p.S);
    int kr_ = tap / p.S, ks_ = tap - kr_ * p.S;
    int nh = max(0, min(p.OH - 1, p.H - 1 + p.pad - kr_) - max(0, p.pad - kr_) + 1);
    int nw = max(0, min(p.OW - 1, p.W - 1 + p.pad - ks_) - max(0, p.pad - ks_) + 1);
    int Meff = p.N * nh * nw;
    int mps = ((Meff + p.splits - 1) / p.splits + 63) / 64 * 64;
    int tile_n = t / ncb, cb = t - tile_n * ncb;
    wgrad256_p8_tile<4096, SCHED>(p, tap * ncb + cb, tile_n, split, true, max(0, p.pad - kr_), max(0, p.pad - ks_), nw, nh * nw, Meff, mps, smem);
  } else {
    wgrad256_p8_tile<4096, SCHED>(p, t % p.tiles_k, t / p.tiles_k, split, false, 0, 0, p.OW, p.OHW, p.M, p.m_per_split, smem);
  }
}

template <int SCHED>
static int wgrad256_group_launch_t(const WgradGroupArgs& g, int slots_per_xcd, hipStream_t st) {
  size_t lds = 8 * 64 * 256 + 4 * 4096;      // operand stages + a 4096-entry pixel -> input offset table
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)conv_wgrad256_group_kernel<SCHED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  conv_wgrad256_group_kernel<SCHED><<<slots_per_xcd * 8, 512, lds, st>>>(g);
  UNIT_LAUNCH_CHECK();
  return UNIT_OK;
}

int unit_wgrad256_group_launch(const WgradGroupArgs& g, int slots_per_xcd, hipStream_t st) {
  switch (wgrad256_loop_sched()) {
    case 0: return wgrad256_group_launch_t<0>(g, slots_per_xcd, st);
    default: return wgrad256_group_launch_t<1>(g, slots_per_xcd, st);
  }
}
