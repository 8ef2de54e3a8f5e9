// The 16-bit direct weight gradient: the templated body of the dad_wgrad_direct* kernels.  The including unit
// (wgrad_direct.hip, wgrad_direct_rg.hip) defines the stamp macros WGD_CLK(), WGD_ACC(k, v) and WGD_ZERO() first
// (whether the stamps build records anything is its choice), then names its kernels with WGD_KERNEL[_CP].
#pragma once
#include <type_traits>

#include "wgrad_common.h"
#include "dad_prep.h"

// ------------------------------------------------------- FP16 / BF16 (throughput modes)
// Direct split-K GEMM after the losses: dW1 = sum_rows G[row]^T x[row] with
//   G[row][h] = ReLU'(row, h) * valid(row) * dL/de_u[h] / max(1, len_u)      (u = row's utterance)
// x is the encoder's 16-bit copy of the student's MFMA input (clean rows, then the
// strong-augmented rows), so one loop with one load type covers both branches.
// One workgroup per (column block of WGD_DB d, split of the slab list), two groups of 4 waves
// (two waves per SIMD): the groups take alternate slabs of the split and their accumulators
// are summed through LDS at the end.  Wave w of a group owns h tiles {2w, 2w+1} x both
// 32-wide d tiles.  Per 32-row slab:
//   x -> LDS [32][WGD_DB] (192-B row pitch: the four rows of a transposed read land on
//     disjoint bank quarters), read as k-major B fragments with ds_read_b64_tr_b16;
//   G is never staged: each lane loads the ReLU' row masks (one u32 per h) of its own two
//     hidden units straight into registers, and its A fragment (8 rows of one h) is byte
//     (16 ks + 8 (lane/32)) of that mask, expanded through a 256-entry LDS table into four
//     0xFFFF/0 dword masks and AND-ed with the 16-bit dL/de_u[h] / len_u in both halves: one
//     bitfield extract, one table read and four ANDs per fragment.  (The loop is bound by
//     vector issue, about ten VALU instructions per MFMA, so table reads replace arithmetic.)
// FP16: the per-utterance scales of hidden unit h are stored as fp16(v * 2^s_h), one power of
// two per h (its largest |v| over the split's utterances maps into [2^14, 2^15): 11 significant
// bits and no overflow or subnormals for values within 2^-28 of the largest), and row h of the
// partial is multiplied by 2^-s_h (exact) before it is stored.
// (The encoder's ping-pong schedule -- one group multiplies under s_setprio while the other builds
// operands, one barrier per phase -- measured slower here in round 5: 29.5-30.1 against 23.2-23.8
// us; a phase of 8 MFMAs is 256 cycles, and the barrier per phase cost more than the overlap won:
// stamps per round 250 operand + 412 MFMA cycles and ~880 waiting at the two barriers.)
// Software pipeline, one barrier per TWO rounds: round j computes slab j from LDS buffer j&3
// while it stages slab j+2 into buffer (j+2)&3 and issues the loads of slab j+2+WGD_DEPTH,
// all in one basic block so the staging VALU fills the MFMA gaps.  dL/de_u[h] / len_u of the
// workgroup's utterances is rebuilt in the prologue (fused_ge1) while the first loads are in
// flight.  Output: one f32 partial slab per split, summed in fixed order by dad_reduce_w.
static_assert(WGD_THREADS == 256 * WGD_GROUPS && DAD_H == 256, "dad_wgrad_direct: groups of 256 threads, thread = h");
static_assert(WGD_GROUPS == 1 || WGD_GROUPS == 2, "dad_wgrad_direct: one or two slab groups");
static_assert(WGD_DB == 64 && DAD_D % WGD_DB == 0, "dad_wgrad_direct: 8 threads x 8 columns per row");
// what a launch converts of the NEXT step's clean rows besides its GEMM (wgd_tile, CP)
enum WgdCp {
  WGD_CP_NONE,      // nothing: the step does not name its next batch
  WGD_CP_PADDED,    // a padded next batch
  WGD_CP_STORE,     // a store batch (Bc <= 64): source rows through the utterance table held in registers
  WGD_CP_STORE16,   // ... whose rows are read from an fp16 / bf16 store in place (the `_s16` kernels)
};

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// B fragment (k-major) of the x tile: 8 x 16-bit in a bf16x8 register container
__device__ __forceinline__ bf16x8 tr_frag(const uint16_t* tile, int pitch, int rowbase, int colbase) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, li = lane & 15;
  const int q = li >> 2, p = li & 3;
  const int col = colbase + 16 * (g & 1) + 4 * p;
  const int row = rowbase + 8 * (g >> 1) + q;
  const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + row * pitch + col));
  const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tile + (row + 4) * pitch + col));
  // one concatenation (a register-pair sequence), not eight element copies
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 c = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, c);
}

// one slab in flight: group thread t holds 8 consecutive columns of row t/8 (staged to LDS
// for everyone) and the ReLU' row masks of its own A-fragment hidden units (kept in
// registers); the slab's utterance slot and valid row count are wave-uniform
struct WgdSlab {
  u32x4 x;
  uint32_t mw[2];
  int ul, nvalid;
};

// Loop-invariant lane offsets and buffer resources of one tile (WGD_V2): every per-slab address of
// the loop is then a scalar (SGPR) base plus one of these, so the loads, the LDS staging and the
// table reads cost no vector instructions for their addresses (the loop is bound by vector issue).
struct WgdLane {
  uint32_t xoff;     // byte offset of this thread's 16 B of x in a 32-row slab of the prepared set
  uint32_t moff;     // byte offset of this lane's row-mask word in a slab's [H] u32 block (m = 0; m = 1 +128)
  uint32_t lsel[2];  // v_perm selectors of the byte of the mask word an A fragment uses (ks = 0, 1),
                     // merged with the lane's 16-B table slot offset (wgd_amask)
  uint32_t slot;     // (lane & 15) * 16: the lane's table slot
  uint32_t gsoff;    // byte offset of this lane's dL/de value in a utterance's [H] row of gs (m = 0)
  int nrows;         // rows of the clean + strong parts of the prepared set (x reads past them read 0)
};

// Slab table of one group, one slab per lane: lane l describes the group's slab j = l,
// global slab s0 + grp + WGD_GROUPS l (clean slabs first, then strong): its first x row (rows of the
// 16-bit copy: clean [b][Tc], then strong [b][Tn]) and (utterance slot << 8 | valid rows).
// A load reads its slab's entry with v_readlane, so no cursor arithmetic runs per slab.
struct WgdTable {
  int row0, info;
  int sd;   // RG: the slab's dense index (its row of the ReLU' mask buffer)
};

__device__ __forceinline__ WgdTable wgd_table(const DadGeom& g, int s, int u0) {
  const SlabIdx q = wg_slab(g, s);
  const bool br = q.br;
  const int b = q.b, c = q.c, T = br ? g.Tn : g.Tc;
  WgdTable t;
  t.row0 = (br ? g.Bc * g.Tc + b * T : b * T) + c * DAD_SLAB;
  t.info = (((br ? g.Bc + b : b) - u0) << 8) | min(T - c * DAD_SLAB, DAD_SLAB);
  t.sd = s;
  return t;
}
// RG (the ragged step, wgrad_direct_rg.hip): the lane's slab is live index k of the student list (live clean, then
// live strong slabs; ps / pz: the live prefixes of dad_common.h over the n list utterances, in LDS).  The
// utterance slot counts the utterances WITH a live slab from the split's first on (pz - zfirst), by order
// of appearance: utterances of length 0 between two live ones take no slot of the LDS dL/de table.
__device__ __forceinline__ WgdTable wgd_table_rg(const DadGeom& g, const int* ps, const int* pz, int n, int k,
                                                 int zfirst) {
  const int u = dad_live_find(ps, n, k), c = k - ps[u];
  const bool br = u >= g.Bc;
  const int b = br ? u - g.Bc : u;
  const int T = br ? g.Tn : g.Tc;
  WgdTable t;
  t.row0 = (br ? g.Bc * g.Tc + b * T : b * T) + c * DAD_SLAB;
  t.info = ((pz[u] - zfirst) << 8) | min(T - c * DAD_SLAB, DAD_SLAB);
  t.sd = br ? g.Bc * g.ncc + b * g.ncn + c : b * g.ncc + c;
  return t;
}


// group slab j: its x rows through a buffer resource of the slab's 32 rows (SGPR base: rows past the
// clean + strong parts read 0, rows past the utterance are the next utterance's prepared rows; both
// are finite and meet mask bits 0, so no clamp runs per slab) and this lane's two row masks
// (buffer loads at the slab's scalar offset)
// RG: the rows past the padded length T read 0 as well (in the dense step they are the next utterance's
// prepared rows; a ragged set holds none for an utterance without frames), and the mask words sit at the
// slab's dense index.
template <bool RG = false>
__device__ __forceinline__ void wgd_load(const DadWgradArgs& a, const WgdTable& tab, int j, int sfirst,
                                          const WgdLane& ln, WgdSlab& r) {
  const int row0 = __builtin_amdgcn_readlane(tab.row0, j);
  const int info = __builtin_amdgcn_readlane(tab.info, j);
  r.ul = info >> 8;
  r.nvalid = 0;
  int n = min(__builtin_amdgcn_readfirstlane(ln.nrows) - row0, DAD_SLAB);   // (uniform: SGPR rsrc)
  if constexpr (RG) n = min(n, info & 0xff);
  const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.xs16 + (size_t)row0 * DAD_D), (short)0,
                                                    n * DAD_D * 2, 0x00020000);
  r.x = __builtin_amdgcn_raw_buffer_load_b128(rx, ln.xoff, 0, 0);
  const auto rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.bits), (short)0, -1, 0x00020000);
  const int soff = (RG ? __builtin_amdgcn_readlane(tab.sd, j) : sfirst + WGD_GROUPS * j) * DAD_H * 4;
  r.mw[0] = __builtin_amdgcn_raw_buffer_load_b32(rb, ln.moff, soff, 0);
  r.mw[1] = __builtin_amdgcn_raw_buffer_load_b32(rb, ln.moff + 128, soff, 0);
}

__device__ __forceinline__ void wgd_stage(const WgdSlab& r, uint16_t* Xt) {
  const int tid = threadIdx.x & 255;
  const int row = tid >> 3;
  // rows past the utterance hold a copy of its last row (finite); their ReLU' mask bits are 0
  *reinterpret_cast<u32x4*>(&Xt[row * WGD_XP + (tid & 7) * 8]) = r.x;
}

// A fragment of h tile ht, k rows 16 ks + 8 (lane/32) + 0..7: bit ? gb : 0 (16-bit pattern).
// lut[b][s] = the 0xFFFF/0 halfword masks of the 8 bits of byte b (16 B), once per 16-B bank
// slot s (64 KB): lane l reads slot l & 15, which is a different slot for every lane of each
// ds_read_b128 lane group ({0-3,12-15,20-27}, {4-11,16-19,28-31}, and +32), so the
// data-dependent bytes never meet on a bank (one table with one copy: 27 % of the kernel's
// LDS cycles were bank conflicts).  One bitfield extract and one 16-B LDS read per fragment.
constexpr int WGD_LUT_SLOTS = 16;
constexpr int WGD_LUT = 256 * WGD_LUT_SLOTS;
// WGD_V2 table: lut[b][s] holds v_perm SELECTORS instead of halfword masks: dword p of the A fragment
// is v_perm(g, g, sel) with sel taking bytes 0, 1 of g (the 16-bit dL/de_u[h] / len_u) into the
// halfword of each set bit (row 2p: bits 0-15, row 2p + 1: bits 16-31) and the zero byte (0x0c)
// into the others.  One v_perm per dword replaces the AND with a g | g << 16 pair, and the
// table address is one v_perm too: byte (2 ks + lane / 32) of the mask word into bits 8-15, the
// lane's slot offset into bits 0-7 (lsel).
__device__ __forceinline__ uint4 wgd_amask(uint32_t mask, const uint4* lut, uint32_t lsel, uint32_t slot) {
  const uint32_t off = __builtin_amdgcn_perm(mask, slot, lsel);   // (mask byte << 8) | (lane & 15) * 16
  return *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(lut) + off);
}

// one slab's operands for one wave: A (G) fragments a[ks][m], B (x) fragments b[ks][n]
struct WgdFrag {
  bf16x8 a[2][2], b[2][2];
};

// the LDS reads of one slab's operands, issued together at the start of a round: B fragments
// (final), the A fragments' table masks and the dL/de pair (combined by wgd_finish at the
// round's end, after the MFMAs have covered the read latency)
struct WgdRaw {
  bf16x8 b[2][2];
  uint4 am[2][2];
  uint32_t gp[2];
};

__device__ __forceinline__ WgdRaw wgd_read(const uint16_t* Xt, const uint32_t (&mk)[2], const uint4* lut,
                                            const uint16_t* gs, int ul, const WgdLane& ln) {
  WgdRaw w;
  const uint16_t* gl = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(gs) + ln.gsoff) + ul * DAD_H;
#pragma unroll
  for (int m = 0; m < 2; ++m) w.gp[m] = gl[32 * m];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int n = 0; n < 2; ++n) w.b[ks][n] = tr_frag(Xt, WGD_XP, 16 * ks, 32 * n);
#pragma unroll
    for (int m = 0; m < 2; ++m) w.am[ks][m] = wgd_amask(mk[m], lut, ln.lsel[ks], ln.slot);
  }
  return w;
}
__device__ __forceinline__ WgdFrag wgd_finish(const WgdRaw& w) {
  WgdFrag f;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint4 s = w.am[ks][m];
      const uint32_t g = w.gp[m];
      f.a[ks][m] = __builtin_bit_cast(bf16x8, uint4{__builtin_amdgcn_perm(g, g, s.x), __builtin_amdgcn_perm(g, g, s.y),
                                                    __builtin_amdgcn_perm(g, g, s.z), __builtin_amdgcn_perm(g, g, s.w)});
    }
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int n = 0; n < 2; ++n) f.b[ks][n] = w.b[ks][n];
  return f;
}

template <bool F16>
__device__ __forceinline__ void wgd_mma(const WgdFrag& f, f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if constexpr (F16)
          acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, f.a[ks][m]),
                                                             __builtin_bit_cast(f16x8, f.b[ks][n]), acc[m][n], 0, 0, 0);
        else
          acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[ks][m], f.b[ks][n], acc[m][n], 0, 0, 0);
      }
}

__device__ __forceinline__ int wgd_utt(const DadGeom& g, int s) {
  const int nsc = g.Bc * g.ncc;
  return s < nsc ? s / g.ncc : g.Bc + (s - nsc) / g.ncn;
}

// power of two 2^s with max_abs * 2^s in [2^14, 2^15) (1 for 0 or a non-finite max)
__device__ __forceinline__ int wgd_f16_exp(float max_abs) {
  if (!(max_abs > 0.0f) || !__builtin_isfinite(max_abs)) return 0;
  int e = 0;
  (void)frexpf(max_abs, &e);   // max_abs = f 2^e, f in [0.5, 1)
  return min(max(15 - e, -126), 126);
}

}  // namespace

// dad_prep_clean_load / _store with the row's address in SGPRs (u is wave-uniform): a buffer
// resource per row, the lane's column offset a loop-invariant register, the three 16-B / 8-B
// pieces at immediate offsets; non-temporal loads as in dad_prep_clean_load.  S: the clean rows'
// source type (DadSrc; a 16-bit store row is 1536 B, its pieces 8 B at 512 k + 8 lane)
// RG (ragged next batch, a store batch): a clean row of a dead slab, t >= 32 ceil(len_b / 32), gets a
// resource of 0 bytes for its load and for its store: the loads return 0 without a memory access and the
// stores are dropped by the range check, with no condition inside the pipelined loop.
__device__ __forceinline__ bool wgd_cp_live(const DadPrepArgs& a, int uc, const StoreRowsW& sr) {
  const int b = sr.tmag ? (int)__umulhi((uint32_t)uc, sr.tmag) : uc;
  const int t = uc - b * a.g.Tc;
  return t < DAD_SLAB * dad_live_slabs(__builtin_amdgcn_readlane(sr.len, b), a.g.ncc);
}
template <bool STORE, typename S, bool RG = false>
__device__ __forceinline__ void wgd_cp_load(const DadPrepArgs& a, int u, uint32_t loff, typename DadSrc<S>::raw (&v)[3],
                                            const StoreRowsW& sr) {
  const int uc = min(u, a.g.Bc * a.g.Tc - 1);
  const size_t srow = dad_clean_src_row<STORE>(a, uc, sr);
  const int bytes = !RG || wgd_cp_live(a, uc, sr) ? DAD_D * (int)sizeof(S) : 0;
  const auto r = __builtin_amdgcn_make_buffer_rsrc(const_cast<S*>(static_cast<const S*>(a.xc) + srow * DAD_D), (short)0,
                                                   bytes, 0x00020000);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if constexpr (sizeof(S) == 4)
      v[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, loff + 1024 * k, 0, 2));
    else
      v[k] = __builtin_amdgcn_raw_buffer_load_b64(r, loff + 512 * k, 0, 2);
  }
}
template <bool F16, typename S, bool RG = false>
__device__ __forceinline__ void wgd_cp_store(const DadPrepArgs& a, int u, uint32_t soff,
                                             const typename DadSrc<S>::raw (&v)[3], const StoreRowsW& sr = StoreRowsW{}) {
  const int uc = min(u, a.g.Bc * a.g.Tc - 1);
  const int bytes = !RG || wgd_cp_live(a, uc, sr) ? DAD_D * 2 : 0;
  const auto r = __builtin_amdgcn_make_buffer_rsrc(a.x16 + (size_t)uc * DAD_D, (short)0, bytes, 0x00020000);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint2 o = dad_src_pack<F16, S>(v[k]);
    __builtin_amdgcn_raw_buffer_store_b64(u32x2{o.x, o.y}, r, soff + 512 * k, 0, 0);
  }
}

// x-tile LDS buffers per slab group: a slab is staged two rounds before it is read, one barrier
// per two rounds (eight buffers and a barrier every four rounds measured neutral, round 3)
constexpr int WGD_NBUF = 4;
// LDS of the weight-gradient workgroups (160 KB with the dL/de table): the x tiles, then the
// mask table; the end-of-tile exchange (red, 64 KB) reuses the x tiles and the spare space
// after them (the table stays intact for the next tile)
constexpr int WGD_XT = WGD_GROUPS * WGD_NBUF * DAD_SLAB * WGD_XP;   // 16-bit elements
constexpr int WGD_RED = WGD_GROUPS == 2 ? DAD_H * WGD_DB : 1;
struct __attribute__((aligned(16))) WgdSmem {
  uint4 lut[WGD_LUT];   // first: its 64 KB sit at LDS offsets 0 .. 65535, so a table read needs no base add
                        // (the ds_read offset field holds 16 bits)
  union {
    uint16_t xt[WGD_XT];
    float red[WGD_RED];
  } a;
};

// what the calls of wgd_tile share besides the launch's arguments and the workgroup's LDS (S, and the dL/de
// table gs: LDS pointers held in a struct compile to generic accesses)
struct WgdCtx {
  int s0, s1, dbase;   // the tile: slabs [s0, s1), columns dbase .. dbase + WGD_DB - 1
  float* outf;         // the split's partial
  int gw, GW;          // CP: this wave's index among the GW waves that convert
  const int* lps;      // RG: the live prefixes over the ln_ list utterances
  const int* lpz;
  int ln_;
};

// one 256 h x WGD_DB d tile over slabs [s0, s1): fp32 partial
// CP: this launch also converts the NEXT step's clean rows into its prepared set (pc, when the
// step names its next batch): wave gw of GW takes rows gw, gw + GW, ...; two rows' loads go out in
// the first round of each block of NB rounds and are converted and stored at the start of the next
// block (an HBM miss under this load takes about as long as NB rounds); the rows left after the
// loop follow it.  CP (WgdCp): a padded next batch, or a store batch (Bc <= 64), source rows through
// the utterance table held in registers (StoreRowsW), rows of type SC (a 16-bit store is read in place).
// RG (the ragged step): [s0, s1) is a range of the live student list, lps / lpz its live prefixes over the
// ln_ list utterances (in the x tiles' LDS, read in the prologue only, before the first slab is staged).
template <bool F16, WgdCp CP, typename SC, bool RG>
__device__ __forceinline__ void wgd_tile(const DadWgradArgs& a, const DadReduceArgs& ra, const DadPrepArgs& pc,
                                         const WgdCtx& t, WgdSmem& S, uint16_t* gs) {
  uint16_t* const Xt = S.a.xt;
  const uint4* const lut = S.lut;
  float* const red = S.a.red;
  const int s0 = t.s0, s1 = t.s1, dbase = t.dbase, gw = t.gw, GW = t.GW, ln_ = t.ln_;
  float* const outf = t.outf;
  const int* const lps = t.lps;
  const int* const lpz = t.lpz;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
  const int grp = __builtin_amdgcn_readfirstlane(tid >> 8);
  const DadGeom& g = a.g;
  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = f32x16{};
  float unscale = 1.0f;   // FP16: 2^-s_h of row h = 64 wv + lane
  const uint32_t cploff = (uint32_t)lane * (4u * sizeof(SC)), cpsoff = (uint32_t)lane * 8u;   // CP: a row's lane columns
  typedef typename DadSrc<SC>::raw CpRaw;
  WGD_ZERO();
  const unsigned long long t0 = WGD_CLK();
  unsigned long long t1 = t0, t2 = t0;
  if (s0 < s1) {
    // group g takes slabs s0 + g, s0 + g + WGD_GROUPS, ...; all groups run nround rounds
    // (barriers); cntmin = the smallest group's slab count
    const int n = s1 - s0;
    const int nround = (n + WGD_GROUPS - 1) / WGD_GROUPS;
    const int mine = (n - grp + WGD_GROUPS - 1) / WGD_GROUPS;   // group 1 may have one slab fewer
    const int cntmin = n / WGD_GROUPS;
    // RG: the split's utterances are those with a live slab from its first slab's on, slot i = the i-th
    // of them (lane i of uslot; at most WGD_MAXU: a range holds at most WGD_MAXU slabs)
    int u0, nu, zfirst = 0, uslot = 0;
    if constexpr (RG) {
      zfirst = lpz[dad_live_find(lps, ln_, s0)];
      nu = lpz[dad_live_find(lps, ln_, s1 - 1)] - zfirst + 1;
      u0 = 0;
      uslot = dad_live_find(lpz, ln_, zfirst + min(lane, nu - 1));
    } else {
      u0 = wgd_utt(g, s0);
      nu = wgd_utt(g, s1 - 1) - u0 + 1;
    }
    auto utt = [&](int i) { return RG ? __builtin_amdgcn_readlane(uslot, i) : u0 + i; };   // (i wave-uniform)
    uint16_t* Xg = Xt + grp * (WGD_NBUF * DAD_SLAB * WGD_XP);   // this group's WGD_NBUF LDS buffers
    // dL/de_u[h] / max(1, len_u) of this split's utterances (thread = h of each group) as 16-bit;
    // the host bounds a split to WGD_MAXU slabs, hence utterances.  In each batch of eight
    // utterances group g builds entries 4g .. 4g+3 (KG per group).  The first batch's vector
    // loads (dL/dz, ECDA row and flag, length) go out before the slab prefetch, so their math
    // never waits on it.
    // FP16: row h of G is stored as fp16(v * 2^s_h), with 2^s_h putting max_u |v[u][h]| in
    // [2^14, 2^15) (wgd_f16_exp); both groups evaluate all KL = 8 utterances of a batch for that
    // max (the same arithmetic: identical s_h in both), so no barrier is needed, and the row
    // of the partial is multiplied back by 2^-s_h when it is stored.  Thread hh is lane hh & 63
    // of wave (hh >> 6) & 3 of its group: the wave that owns rows 64 wv .. 64 wv + 63.
    constexpr int KG = 8 / WGD_GROUPS;
    constexpr int KL = F16 ? 8 : KG;
    auto slot = [&](int k) { return F16 ? k : grp * KG + k; };   // utterance slot of evaluation k
    const int hh = tid & (DAD_H - 1);
    float w2[4], ec0[KL], vl0[KL];
    f32x4 gz0[KL];
    uint32_t ef0[KL];
#pragma unroll
    for (int c = 0; c < 4; ++c) w2[c] = ra.student[DAD_OFF_W2 + c * DAD_H + hh];
#pragma unroll
    for (int k = 0; k < KL; ++k) {
      const int u = utt(min(slot(k), nu - 1));
      ec0[k] = ra.ge_ecda[(size_t)u * DAD_H + hh];
      gz0[k] = *reinterpret_cast<const f32x4*>(ra.gzb + (size_t)u * DAD_C);
      ef0[k] = ra.eflag[u];
      vl0[k] = ra.vlen[u];
    }
    const int sfirst = s0 + grp;
    WgdTable tab;
    if constexpr (RG) {
      tab = wgd_table_rg(g, lps, lpz, ln_, min(sfirst + WGD_GROUPS * lane, s1 - 1), zfirst);
      __syncthreads();   // every wave has read the prefixes: the x tiles may be staged
    } else {
      tab = wgd_table(g, min(sfirst + WGD_GROUPS * lane, s1 - 1), u0);
    }
    WgdLane ln;
    {
      const int t = tid & 255;
      ln.xoff = (uint32_t)(((t >> 3) * DAD_D + dbase + (t & 7) * 8) * 2);
      ln.moff = (uint32_t)(((2 * wv) * 32 + (t & 31)) * 4);
      ln.slot = (uint32_t)(lane & (WGD_LUT_SLOTS - 1)) << 4;
      ln.lsel[0] = 0x0c0c0000u | ((4u + (uint32_t)(lane >> 5)) << 8);   // mask byte 0 / 1 (ks = 0)
      ln.lsel[1] = 0x0c0c0000u | ((6u + (uint32_t)(lane >> 5)) << 8);   // mask byte 2 / 3 (ks = 1)
      ln.gsoff = (uint32_t)(((2 * wv) * 32 + (lane & 31)) * 2);
      ln.nrows = g.Bc * g.Tc + (a.warmup ? 0 : g.Bn * g.Tn);
    }
    const int jlast = max(mine - 1, 0);
    WgdSlab r[WGD_DEPTH];
    // loads are unconditional (slab index clamped at the group's last slab): conditional
    // loads make the compiler merge the paths' pending counts into a vmcnt(0) drain
#pragma unroll
    for (int k = 0; k < WGD_DEPTH; ++k) wgd_load<RG>(a, tab, min(k, jlast), sfirst, ln, r[k]);
    const unsigned long long ta = WGD_CLK();
    // the table: the first batch's values stay in registers (v0); FP16 takes the row's largest
    // |v| first (a second pass recomputes later batches), then writes the scaled values
    auto ge_table = [&](auto ex_tag) {
      constexpr bool EX = decltype(ex_tag)::value;
      auto batch = [&](int ul0, float (&v)[KL]) {
#pragma unroll
        for (int k = 0; k < KL; ++k) {   // the batch's loads in flight (index clamped)
          const int u = utt(min(ul0 + slot(k), nu - 1));
          v[k] = ul0 == 0 ? fused_ge1_v<EX>(ra, g.Bc, u, hh, w2, gz0[k], ef0[k], ec0[k]) / fmaxf(vl0[k], 1.0f)
                          : fused_ge1<EX>(ra, g.Bc, u, hh, w2) / fmaxf(ra.vlen[u], 1.0f);
        }
      };
      auto put = [&](int ul0, const float (&v)[KL], float scale) {
#pragma unroll
        for (int k = 0; k < KG; ++k) {
          const int uk = ul0 + grp * KG + k;
          const float x = v[F16 ? grp * KG + k : k];
          if (uk < nu) gs[uk * DAD_H + hh] = dad_half_bits(F16 ? x * scale : x, F16);
        }
      };
      float v0[KL];
      batch(0, v0);
      float scale = 1.0f;
      if constexpr (F16) {
        float mx = 0.0f;
#pragma unroll
        for (int k = 0; k < KL; ++k) mx = fmaxf(mx, fabsf(v0[k]));   // (clamped slots repeat a real one)
        for (int ul0 = 8; ul0 < nu; ul0 += 8) {
          float v[KL];
          batch(ul0, v);
#pragma unroll
          for (int k = 0; k < KL; ++k) mx = fmaxf(mx, ul0 + k < nu ? fabsf(v[k]) : 0.0f);
        }
        const int s = wgd_f16_exp(mx);
        scale = __builtin_ldexpf(1.0f, s);
        unscale = __builtin_ldexpf(1.0f, -s);
      }
      put(0, v0, scale);
      for (int ul0 = 8; ul0 < nu; ul0 += 8) {
        float v[KL];
        batch(ul0, v);
        put(ul0, v, scale);
      }
    };
    if (ra.keep1) ge_table(std::true_type{});
    else ge_table(std::false_type{});
    const unsigned long long tb = WGD_CLK();
    // slabs 0 .. SD-1 of each group into buffers 0 .. SD-1; their ring slots reload slabs
    // WGD_DEPTH .. WGD_DEPTH + SD - 1
    constexpr int NB = WGD_NBUF, SD = WGD_NBUF / 2;   // LDS buffers, staging distance (rounds)
    static_assert(WGD_DEPTH == 4 && NB == 4, "dad_wgrad_direct: four ring slots, 4 LDS buffers");
    int ulq[SD];   // utterance slot and row masks of slabs j .. j+SD-1 (by j mod SD)
    uint32_t mwq[SD][2];
#pragma unroll
    for (int q = 0; q < SD; ++q) {
      if (mine > q) wgd_stage(r[q], Xg + q * (DAD_SLAB * WGD_XP));
      ulq[q] = r[q].ul;
      mwq[q][0] = r[q].mw[0];
      mwq[q][1] = r[q].mw[1];
    }
#pragma unroll
    for (int q = 0; q < SD; ++q) wgd_load<RG>(a, tab, min(WGD_DEPTH + q, jlast), sfirst, ln, r[q]);
    const unsigned long long tc = WGD_CLK();
    __syncthreads();
    t1 = WGD_CLK();
    WGD_ACC(3, ta - t0); WGD_ACC(6, tb - ta); WGD_ACC(7, tc - tb); (void)ta; (void)tb; (void)tc;
    // round j: read slab j's operands from buffer j % NB into registers | MFMAs of slab j-1 from
    // the registers read in round j-1 (so they never wait on LDS) | stage slab j+SD into
    // buffer (j+SD) % NB from ring slot (j+SD) % 4 and reload that slot with slab j+SD+4.  A slab
    // is staged SD = NB/2 rounds before it is read, so one barrier per SD rounds (after rounds
    // j = SD-1 mod SD) orders every staging before its reads and every read before its buffer is
    // restaged.
    WgdFrag F;
    auto round = [&](int jr, int k, bool prev, bool comp, bool stage, bool bar) {
      const unsigned long long c0 = WGD_CLK();
      const int nk = (k + SD) % WGD_DEPTH;
      WgdRaw R;
      if (comp) R = wgd_read(Xg + (k % NB) * (DAD_SLAB * WGD_XP), mwq[k % SD], lut, gs, ulq[k % SD], ln);
      __builtin_amdgcn_sched_barrier(0);   // reads first, their latency under the MFMAs
      if (prev) wgd_mma<F16>(F, acc);
      if (stage) wgd_stage(r[nk], Xg + ((k + SD) % NB) * (DAD_SLAB * WGD_XP));
      ulq[k % SD] = r[nk].ul;
      mwq[k % SD][0] = r[nk].mw[0];
      mwq[k % SD][1] = r[nk].mw[1];
      wgd_load<RG>(a, tab, min(jr + SD + WGD_DEPTH, jlast), sfirst, ln, r[nk]);
      __builtin_amdgcn_sched_barrier(0);
      if (comp) F = wgd_finish(R);
      const unsigned long long c1 = WGD_CLK();
      if (bar) __syncthreads();
      WGD_ACC(4, c1 - c0); WGD_ACC(5, WGD_CLK() - c1); WGD_ACC(8, 1);
      (void)c0; (void)c1;
    };
    // round 0, then blocks of NB rounds (NB is a multiple of the 4 ring slots) in which both
    // groups have every step (no early exits: an exit inside the block would reach the loop
    // header with a different load order and force vmcnt(0) there; buffers and ring slots are
    // compile-time: j = 1 mod NB at a block start), then the last rounds with per-group flags and
    // the final MFMAs.  Both groups run the same rounds, so the barriers match.
    round(0, 0, false, mine > 0, SD < mine, false);
    int j = 1;
    int prow = gw;        // CP: this wave's next clean row of the next step
    const StoreRowsW srw = CP == WGD_CP_STORE ? dad_store_rows_w(pc, lane) : StoreRowsW{};
    CpRaw pv[2][3];
    bool pending = false; // CP: rows prow - 2 GW, prow - GW loaded, not yet stored
    CpRaw po[2][3];       // CP two blocks ahead: rows prow - 4 GW, prow - 3 GW (loaded two blocks ago)
    bool pend2 = false;
    for (; j + NB - 1 + SD < cntmin; j += NB) {   // every round stages slab j + k + SD < cntmin
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        if constexpr (CP != WGD_CP_NONE) {
          if (k == 0) {
            // the rows loaded two blocks (2 NB rounds) ago, then this block's two
            if (pend2) {
              wgd_cp_store<F16, SC, RG>(pc, prow - 4 * GW, cpsoff, po[0], srw);
              wgd_cp_store<F16, SC, RG>(pc, prow - 3 * GW, cpsoff, po[1], srw);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
              for (int e = 0; e < 3; ++e) po[q][e] = pv[q][e];
            pend2 = pending;
            wgd_cp_load<CP == WGD_CP_STORE, SC, RG>(pc, prow, cploff, pv[0], srw);
            wgd_cp_load<CP == WGD_CP_STORE, SC, RG>(pc, prow + GW, cploff, pv[1], srw);
            prow += 2 * GW;
            pending = true;
          }
        }
        round(j + k, (k + 1) % NB, true, true, true, (k + 1) % SD == SD - 1);
      }
    }
#pragma unroll
    for (int k = 0; k < NB + SD + 1; ++k)   // nround - j <= NB + SD
      if (j + k < nround)
        round(j + k, (k + 1) % NB, j + k - 1 < mine, j + k < mine, j + k + SD < mine, (k + 1) % SD == SD - 1);
    if (nround - 1 < mine) wgd_mma<F16>(F, acc);
    if constexpr (CP != WGD_CP_NONE) {
      if (pend2) {
        wgd_cp_store<F16, SC, RG>(pc, prow - 4 * GW, cpsoff, po[0], srw);
        wgd_cp_store<F16, SC, RG>(pc, prow - 3 * GW, cpsoff, po[1], srw);
      }
      if (pending) {
        wgd_cp_store<F16, SC, RG>(pc, prow - 2 * GW, cpsoff, pv[0], srw);
        wgd_cp_store<F16, SC, RG>(pc, prow - GW, cpsoff, pv[1], srw);
      }
      for (; prow < pc.g.Bc * pc.g.Tc; prow += GW) {   // the rows the loop left
        wgd_cp_load<CP == WGD_CP_STORE, SC, RG>(pc, prow, cploff, pv[0], srw);
        wgd_cp_store<F16, SC, RG>(pc, prow, cpsoff, pv[0], srw);
      }
    }
    t2 = WGD_CLK();
  } else if constexpr (CP != WGD_CP_NONE) {
    const StoreRowsW srw = CP == WGD_CP_STORE ? dad_store_rows_w(pc, lane) : StoreRowsW{};
    for (int prow = gw; prow < pc.g.Bc * pc.g.Tc; prow += GW) {
      CpRaw pv[3];
      wgd_cp_load<CP == WGD_CP_STORE, SC, RG>(pc, prow, cploff, pv, srw);
      wgd_cp_store<F16, SC, RG>(pc, prow, cpsoff, pv, srw);
    }
  }
  const int kh = lane >> 5;
  if constexpr (WGD_GROUPS == 2) {
    __syncthreads();   // red aliases the x tiles: every group's last reads are done
    // exchange halves: group 0 finishes h tile 2w (+ group 1's partial), group 1 tile 2w+1
#pragma unroll
    for (int m = 0; m < 2; ++m)
      if (m != grp)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int rr = 0; rr < 16; ++rr)
            red[((2 * wv + m) * 32 + dad_acc_row(rr, kh)) * WGD_DB + 32 * nn + (lane & 31)] = acc[m][nn][rr];
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
    if (WGD_GROUPS == 1 || m == grp)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          const int h = (2 * wv + m) * 32 + dad_acc_row(rr, kh);
          const int d = 32 * nn + (lane & 31);
          const float v = acc[m][nn][rr] + (WGD_GROUPS == 2 ? red[h * WGD_DB + d] : 0.0f);
          // FP16: 2^-s_h of row h, held by lane h - 64 wv of this wave (ds_bpermute)
          outf[(size_t)h * DAD_D + dbase + d] = F16 ? v * __shfl(unscale, h - 64 * wv, 64) : v;
        }
  if constexpr (WGD_GROUPS == 2) __syncthreads();   // red free for the next tile
  WGD_ACC(0, t1 - t0); WGD_ACC(1, t2 - t1); WGD_ACC(2, WGD_CLK() - t2);
  (void)t0; (void)t1; (void)t2;
}

// the byte table of the A-fragment masks, 16 slot copies per byte (wgd_amask)
__device__ __forceinline__ void wgd_lut(uint4* lut) {
  // consecutive threads store consecutive 16-B slots (conflict-free stores); entry i is byte
  // i / 16, the byte's four dwords by sign-extended bit fields
#pragma unroll
  for (int k = 0; k < (WGD_LUT + WGD_THREADS - 1) / WGD_THREADS; ++k) {
    const int i = k * WGD_THREADS + threadIdx.x;
    if (WGD_LUT < WGD_THREADS && i >= WGD_LUT) break;
    const int t = i / WGD_LUT_SLOTS;
    uint32_t e[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      e[p] = (((t >> (2 * p)) & 1) ? 0x00000100u : 0x00000c0cu) | (((t >> (2 * p + 1)) & 1) ? 0x01000000u : 0x0c0c0000u);
    lut[i] = uint4{e[0], e[1], e[2], e[3]};
  }
}

// RG (wgrad_direct_rg.hip, the ragged step): a split's range is its share of the LIVE student list (wg_range's
// formula on the live count: the host chose `splits` from the dense count, so a share holds at most
// WGD_MAXU slabs); the live prefixes are built from the batch's device lengths in the x tiles' LDS.  A
// split whose share is empty writes a zero partial.
template <bool F16, WgdCp CP, bool RG>
__device__ __forceinline__ void wgrad_direct_body(const DadWgradArgs& a, const DadReduceArgs& ra, const DadPrepArgs& pc) {
  __shared__ WgdSmem S;
  __shared__ __attribute__((aligned(16))) uint16_t gs[WGD_MAXU * DAD_H];
  // XCD-aware tile order (grid is a multiple of 8; workgroups go round-robin over the 8
  // XCDs): each XCD takes a consecutive run of tiles, so the column blocks of one split,
  // which read the same ReLU' row masks, share an L2
  const int per_xcd = gridDim.x >> 3;
  const int tile = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (tile >= a.ntiles) {
    // The first WGD_XWG spare workgroups do dad_reduce's extra blocks (db1, dW2, loss totals):
    // their inputs are ready before this launch and the work then overlaps the GEMM instead of
    // trailing the reduction.  Two extra blocks at a time, one per 256-thread half, combining
    // in the (otherwise unused) x-tile LDS.
    const int xi = tile - a.ntiles;
    if (xi >= WGD_XWG) return;
    static_assert(sizeof(S.a) >= 2 * 16 * 16 * 6 * sizeof(float), "extra-block scratch fits the x tile");
    double* wred = reinterpret_cast<double*>(S.lut);   // (the mask table is not used here)
    const int half = threadIdx.x >> 8, htid = threadIdx.x & 255;
    float (*xs)[16][6] = reinterpret_cast<float (*)[16][6]>(S.a.red) + 16 * half;
    constexpr int per_wg = DAD_REDUCE_XBLK / WGD_XWG;
    constexpr int NB = DAD_REDUCE_BLOCKS - DAD_REDUCE_XBLK;
    // (Both iterations unrolled, as the compiler chose by itself when all these kernels and dad_reduce shared
    // a unit, except in dad_wgrad_direct_f16_cps_rg, where it kept the loop: said here, so that the choice no
    // longer follows from which other callers of extra_block a unit holds.)
#pragma unroll(RG && F16 && CP != WGD_CP_NONE ? 1 : 2)
    for (int r = 0; r < per_wg; r += 2) {
      const int e = xi * per_wg + r + half;
      const double v = dad_wave_sum_d(extra_block(ra, e, htid, xs));
      if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = v;
      __syncthreads();
      if (htid == 0 && ra.want_norm)
        ra.normpart[NB + e] = (float)(((wred[4 * half] + wred[4 * half + 1]) + wred[4 * half + 2]) + wred[4 * half + 3]);
      __syncthreads();
    }
    return;
  }
  const int split = tile / WGD_NDB, dblk = tile - split * WGD_NDB;
  int s0, s1;
  const int rg_bn = a.warmup ? 0 : a.g.Bn, rg_n = a.g.Bc + rg_bn;
  int* const lps = reinterpret_cast<int*>(S.a.xt);
  int* const lpss = lps + (rg_n + 1);
  int* const lpz = lpss + (rg_n + 1);
  if constexpr (RG) {
    static_assert(3 * 4 * (2 * DAD_MAX_BATCH + 1) <= sizeof(S.a), "the live prefixes fit the x tiles");
    dad_live_prefix_lds(a.src.lenc, a.g.Bc, a.g.ncc, a.g.Tc, a.src.lenn, rg_bn, a.g.ncn, a.g.Tn, lps, lpss, lpz);
    dad_wg_share(lps[rg_n], a.splits, split, s0, s1);
  } else {
    wg_range(a, split, s0, s1);
  }
  wgd_lut(S.lut);   // (the tile's first barrier orders it before the first read)
  const int gw = __builtin_amdgcn_readfirstlane(tile * (WGD_THREADS / 64) + (int)(threadIdx.x >> 6));
  float* const outf = a.wpart + (size_t)split * DAD_H * DAD_D;
  const int GW = a.ntiles * (WGD_THREADS / 64);
  const WgdCtx t{s0, s1, dblk * WGD_DB, outf, gw, GW, lps, lpz, rg_n};
  // The clean rows' source type, block-uniform.  STORE16, the `_s16` sibling of the store variant, reads an
  // fp16 / bf16 store in its own type: a kernel of its own, so that the f32 kernels hold the f32 code alone.
  // A ragged launch's next batch, ragged too, is a store batch of any of the three types.
  constexpr WgdCp CPT = CP == WGD_CP_STORE16 ? WGD_CP_STORE : CP;
  constexpr bool S16 = CP == WGD_CP_STORE16 || (RG && CP != WGD_CP_NONE), S32 = CP != WGD_CP_STORE16;
  if constexpr (RG) {
    if constexpr (CP != WGD_CP_NONE) {
      if (pc.xc_type() == DAD_STORE_F16)
        wgd_tile<F16, CPT, _Float16, RG>(a, ra, pc, t, S, gs);
      else if (pc.xc_type() == DAD_STORE_BF16)
        wgd_tile<F16, CPT, __bf16, RG>(a, ra, pc, t, S, gs);
      else
        wgd_tile<F16, CPT, float, RG>(a, ra, pc, t, S, gs);
    } else {
      wgd_tile<F16, CPT, float, RG>(a, ra, pc, t, S, gs);
    }
  } else if constexpr (CP == WGD_CP_STORE16) {
    if (pc.xc_type() == DAD_STORE_F16)
      wgd_tile<F16, CPT, _Float16, RG>(a, ra, pc, t, S, gs);
    else
      wgd_tile<F16, CPT, __bf16, RG>(a, ra, pc, t, S, gs);
  } else {
    wgd_tile<F16, CPT, float, RG>(a, ra, pc, t, S, gs);
  }
}

// the entry points: one line each in the including unit (without / with a next batch to convert)
#define WGD_KERNEL(name, F16, RG)                                                                   \
  __global__ __launch_bounds__(WGD_THREADS, 1) void name(DadWgradArgs a, DadReduceArgs ra) {        \
    DAD_GUARD_BLOCK(WGD_THREADS);                                                                   \
    wgrad_direct_body<F16, WGD_CP_NONE, RG>(a, ra, DadPrepArgs{});                                  \
  }
#define WGD_KERNEL_CP(name, F16, CP, RG)                                                                     \
  __global__ __launch_bounds__(WGD_THREADS, 1) void name(DadWgradArgs a, DadReduceArgs ra, DadPrepArgs pc) { \
    DAD_GUARD_BLOCK(WGD_THREADS);                                                                            \
    wgrad_direct_body<F16, CP, RG>(a, ra, pc);                                                               \
  }
