// fp64 tiled GEMM / SYRK for gfx950 on v_mfma_f64_16x16x4_f64 with VGPR accumulators.
//
// Measured on MI355X (profiles/r01_probe_*.txt): v_mfma_f64_16x16x4_f64 issues every 64.0 cycles
// (77.0 TFLOP/s chip-wide, 98 % of the 78.6 TFLOP/s fp64 peak) when its C/D operand lives in VGPRs,
// but every 130 cycles (38 TFLOP/s) when C/D is in AGPRs -- so this library is compiled with
// -mllvm -amdgpu-mfma-vgpr-form.
// Lane maps of the 16x16x4 form (one f64 of A and of B per lane, 4 f64 of C/D per lane):
//   A[i = l&15][k = l>>4]   B[k = l>>4][j = l&15]   D[row = (l>>4) + 4r][col = l&15], r = 0..3
//
// Two kernels, one design (256 threads = 4 waves as 2x2; MFMA operand fragments double-buffered in registers one k4-step
// ahead; branch-free chunk bodies in which sched_group_barrier spreads the memory instructions between the MFMAs; two
// workgroups per CU).  What they share is written once, ahead of them: which k range and batch member a workgroup takes
// (k_range, batch_ptrs), the register-staged operand path (chunk_offsets / chunk_load / chunk_store over
// StageB / StageS) and the k-segment step (kseg_mask, kseg_jump); the host finds every instantiation in GEMM_KERNELS.
//   gemm_f64_kernel_b : 128x128 output tile per workgroup (64x64 per wave = 4x4 MFMA tiles = 64 accumulator doubles per
//                       lane), with two operand paths.
//                       NT form (both operands row-major, the Cholesky's bulk updates): K in chunks of 8 filled global ->
//                       LDS by LDS-DMA (global_load_lds, 16 bytes per lane, no VGPR staging) into four LDS stages of a
//                       row-major, XOR-swizzled image (64 KiB), requested three chunks ahead so that one stays in flight
//                       across every chunk barrier.
//                       Forms with a k-major operand: K in chunks of 16 through a double-buffered k-major LDS image
//                       ([k][x], leading dimension 144 doubles so both halves of a ds_read_b64 wave access hit disjoint
//                       banks, 72 KiB), global -> register prefetch two chunks ahead, registers -> LDS one chunk ahead.
//   gemm_f64_kernel_s : the register-staged schedule on 64x64 tiles (three LDS buffers, 60 KiB) for launches with too few
//                       128x128 tiles to fill the chip; its row-major operands are fetched as whole 128-byte row segments
//                       and stored XOR-swizzled (round 4).
//
// They serve: K3 Cholesky trailing / panel updates (NT, lower), K7 triangular
// inverse levels (NN with triangular k-ranges) and L^-T L^-1 (TN), K8 predict triangular-solve updates (NT).
// (Two rejected designs -- an 8-wave / one-workgroup-per-CU 128x128 kernel with BK = 32, 62 TFLOP/s, and an 8-wave half-CU
// kernel with persistent CU-subset modes, 73 TFLOP/s but no gain next to the panel chain -- lived here in round 1; DESIGN.md
// section 3 and 8 keep what they showed, git history keeps the code.)
#include <cstdlib>
#include <type_traits>
#include "migp_kernels.h"

namespace migp {

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int TILE = 128;
constexpr int LDS_LD = 144;

__device__ __forceinline__ void tile_from_index(int tri, int nt, int idx, int& ti, int& tj) {
  if (tri) {
    const int ntri = nt * (nt + 1) / 2;
    if (idx < ntri) {
      int t = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
      while ((t + 1) * (t + 2) / 2 <= idx) ++t;
      while (t * (t + 1) / 2 > idx) --t;
      ti = t;
      tj = idx - t * (t + 1) / 2;
    } else {
      const int rem = idx - ntri;
      ti = nt + rem / nt;
      tj = rem % nt;
    }
  } else {
    ti = idx / nt;
    tj = idx % nt;
  }
}
__device__ __forceinline__ void tile_from_index(const GemmParams& p, int idx, int& ti, int& tj) {
  tile_from_index(p.tri, p.nt, idx, ti, tj);
}

// Band-column-major enumeration of the lower trapezoid (tri) or the full rectangle: bands of R tile rows; inside a band the columns left to right,
// inside a column the band's rows top to bottom.  The 64 tiles an XCD works on at a time then cover ~R row strips and
// ~64/R column strips (each fetched into that L2 once and hit by the others) instead of one row strip and 64 column strips.
__device__ __forceinline__ void tile_from_index_banded(int tri, int mt, int nt, int idx, int R, int& ti, int& tj) {
  auto before = [&](int r) {  // tiles in tile rows [0, r)
    if (!tri) return r * nt;
    return r <= nt ? r * (r + 1) / 2 : nt * (nt + 1) / 2 + (r - nt) * nt;
  };
  int lo = 0, hi = (mt + R - 1) / R - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (before(mid * R) <= idx) lo = mid; else hi = mid - 1;
  }
  const int r0 = lo * R, r1 = min(r0 + R, mt), h = r1 - r0;
  int e = idx - before(r0);
  const int cfull = tri ? min(r0 + 1, nt) : nt;  // columns that hold all h rows of the band
  if (e < cfull * h) { tj = e / h; ti = r0 + e % h; return; }
  e -= cfull * h;
  for (tj = cfull; tj < nt; ++tj) {    // the band's own triangle: column tj holds rows tj .. r1-1
    const int cnt = r1 - tj;
    if (e < cnt) { ti = tj + e; return; }
    e -= cnt;
  }
  ti = r1 - 1; tj = min(ti, nt - 1);
}

__device__ __forceinline__ void tile_from_index_banded(const GemmParams& p, int idx, int R, int& ti, int& tj) {
  tile_from_index_banded(p.tri, p.mt, p.nt, idx, R, ti, tj);
}

// First-columns-first enumeration of the lower trapezoid (GemmParams::fc): the fc leading tile columns row by row, then the
// sub-trapezoid of the remaining columns in the banded order.
__device__ __forceinline__ void tile_from_index_fc(int mt, int nt, int fc, int band, int idx, int& ti, int& tj) {
  const int ft = fc * (fc + 1) / 2 + (mt - fc) * fc;
  if (idx < ft) {
    tile_from_index(1, fc, idx, ti, tj);
  } else {
    if (band > 0) tile_from_index_banded(1, mt - fc, nt - fc, idx - ft, band, ti, tj);
    else tile_from_index(1, nt - fc, idx - ft, ti, tj);
    ti += fc;
    tj += fc;
  }
}

// Panel-list mode (GemmParams::pl): tile `idx` of the launch -> tile-unit coordinates of its A rows, B rows, C rows and C
// columns, and whether it is a diagonal tile of its panel's trapezoid.  The table walk is uniform per workgroup (scalar loads).
__device__ __forceinline__ void list_tile(const GemmParams& p, int idx, int& ra, int& rb, int& rc, int& cc, bool& diag) {
  const int want = idx + p.pl[p.pl_first].x;
  int lo = p.pl_first, hi = p.pl_first + p.pl_n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.pl[mid].x <= want) lo = mid; else hi = mid - 1;
  }
  const int4 d = p.pl[lo];
  int ti, tj;
  if (p.band > 0) tile_from_index_banded(1, p.pl_rows - d.y, d.w, want - d.x, p.band, ti, tj);
  else tile_from_index(1, d.w, want - d.x, ti, tj);
  ra = d.y - p.pl_abase + ti;
  rb = d.y - p.pl_abase + tj;
  rc = d.y + ti;
  cc = d.z + tj;
  diag = (ti == tj);
}

// ---------------------------------------------------------------------------------------------
// What both kernels share of "which k range, which batch member".  The block -> tile decode (XCD-aware map, the choice
// between the fc / banded / plain orders, the kmode 2 / 4 reversal) stands in each kernel, each copy naming the other: as
// shared functions these moved the scalar code and the scalar register numbering of gemm_f64_kernel_s, whatever the spelling
// (profiles/NOTES_gemm_refactor.md).

// kmode -> the k range [beg, end) of the tile at rows i0, columns j0 (T: tile edge): 0 all of k; 1 / 3 from the tile's own
// column / row on (lower-triangular B / A); 2 / 4 up to the end of the tile's own row / column (lower-triangular A / B^T)
struct KRange { int end, beg; };  // (in this order the kernels' scalar code is the one they had with two locals)
template <int T>
__device__ __forceinline__ KRange k_range(const GemmParams& p, int i0, int j0) {
  KRange r = {p.k, 0};
  if (p.kmode == 1) r.beg = j0;
  else if (p.kmode == 2) r.end = i0 + T;
  else if (p.kmode == 3) r.beg = i0;
  else if (p.kmode == 4) r.end = j0 + T;
  return r;
}

// blockIdx.z = z1 + batch1 * z2 (two-level batch: nodes of a triangular-inverse level x problems of a batched evaluation)
struct BatchPtrs { const double* A; const double* B; double* C; };
__device__ __forceinline__ BatchPtrs batch_ptrs(const GemmParams& p) {
  const long z1 = p.batch1 > 0 ? (long)(blockIdx.z % p.batch1) : (long)blockIdx.z, z2 = p.batch1 > 0 ? (long)(blockIdx.z / p.batch1) : 0;
  return {p.A + z1 * p.strideA + z2 * p.strideA2, p.B + z1 * p.strideB + z2 * p.strideB2, p.C + z1 * p.strideC + z2 * p.strideC2};
}

// A run of sched_group_barrier: (instruction class, count) pairs in issue order -- how a chunk body spreads its memory
// instructions between its MFMAs
constexpr int SG_MFMA = 0x008, SG_VMEM_READ = 0x020, SG_DS_READ = 0x100, SG_DS_WRITE = 0x200;
template <int MASK, int N, int... REST>
__device__ __forceinline__ void sched_groups() {
  __builtin_amdgcn_sched_group_barrier(MASK, N, 0);
  if constexpr (sizeof...(REST) > 0) sched_groups<REST...>();
}

// ---------------------------------------------------------------------------------------------
// Register-staged operand path of both kernels: a chunk of 16 k of one operand goes global -> registers (double2 pieces,
// 256 threads) -> a k-major LDS image [k][x] of leading dimension S::LD.  S names what differs between the kernels:
//   S::T    tile edge: x extent of the chunk (a k-major operand has T / 2 threads per k row, 512 / T k rows per piece)
//   S::LD   leading dimension of the LDS image in doubles
//   S::SWZ  row-major operands: fetch whole 128-byte row segments and XOR-swizzle the image's columns (below)
struct StageB { static constexpr int T = TILE, LD = LDS_LD; static constexpr bool SWZ = false; };
// LD 80 = 64 + 16: odd k rows land 16 bank-pairs away from even ones
struct StageS { static constexpr int T = 64, LD = 80; static constexpr bool SWZ = true; };

template <class S, bool KMAJOR>
__device__ __forceinline__ void chunk_offsets(long ld, int tid, unsigned& goff, unsigned& loff, long& gstride) {
  if (KMAJOR) {
    constexpr int XT = S::T / 2, KR = 256 / XT;  // threads per k row, k rows per piece: k = KR q + tid / XT
    const int k = tid / XT, xc = tid % XT;
    goff = (unsigned)((k * ld + 2 * xc) * 8);
    loff = (unsigned)((k * S::LD + 2 * xc) * 8);
    gstride = KR * ld * 8;
  } else if (S::SWZ) {
    // Eight consecutive lanes fetch ONE row's 128-byte chunk segment (a whole cache line per row, 8 rows per wave
    // instruction) instead of sixteen lanes fetching 16 bytes of sixteen different rows.  The k-major LDS image is then
    // written with the column XOR-swizzled by the k pair, col = x ^ (k & 14): a wave's 16-lane write groups (8 k pairs x 2
    // rows) hit 16 distinct bank pairs, and a fragment read (16 consecutive x at one k, XORed with a constant below 16)
    // stays a permutation of its aligned 16-column block, so the read side keeps its conflict-free pattern.
    const int kc = tid & 7, row = tid >> 3;  // x = 32q + (t>>3), k = 2 (t&7)
    goff = (unsigned)((row * ld + 2 * kc) * 8);
    loff = (unsigned)(((2 * kc) * S::LD + (row ^ (2 * kc))) * 8);
    gstride = 32 * ld * 8;
  } else {
    const int xl = tid & 15, kc = (tid >> 4) & 7, xh = tid >> 7;  // x = 32q + 16*(t>>7) + (t&15)
    goff = (unsigned)(((xh * 16 + xl) * ld + 2 * kc) * 8);
    loff = (unsigned)(((2 * kc) * S::LD + xh * 16 + xl) * 8);
    gstride = 32 * ld * 8;
  }
}
template <int NQ>
__device__ __forceinline__ void chunk_load(const char* __restrict__ base, unsigned goff, long gstride, double2_t (&r)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) r[q] = *reinterpret_cast<const double2_t*>(base + q * gstride + goff);
}
template <class S, bool KMAJOR, int NQ>
__device__ __forceinline__ void chunk_store(char* __restrict__ lds, unsigned loff, const double2_t (&r)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (KMAJOR) {
      *reinterpret_cast<double2_t*>(lds + loff + q * (512 / S::T * S::LD * 8)) = r[q];
    } else {
      *reinterpret_cast<double*>(lds + loff + q * (32 * 8)) = r[q].x;
      *reinterpret_cast<double*>(lds + loff + q * (32 * 8) + S::LD * 8) = r[q].y;
    }
  }
}

// k-segmented operands (GemmParams::kseg; row-major operands only): the byte step INTO chunk n of BK k is kseg_jump, to the
// next segment's base, when n & kseg_mask is 0 (n a multiple of kseg / BK), else the step inside a segment
template <int BK>
__device__ __forceinline__ int kseg_mask(const GemmParams& p) { return p.kseg > 0 ? p.kseg / BK - 1 : 0x7fffffff; }
template <int BK>
__device__ __forceinline__ long kseg_jump(const GemmParams& p) { return (p.kseg_stride - (long)(p.kseg - BK)) * 8; }

// ---------------------------------------------------------------------------------------------
// 128x128 tiles: 256-thread workgroups (4 waves as 2x2, 64x64 per wave = 4x4 MFMA tiles, 64 accumulator
// doubles per lane).  Register path (a k-major operand): K chunks of 16 (BKB), 72 KiB of LDS; LDS-DMA path (NT form): K
// chunks of 8 (BKD), four stages, 64 KiB.  Either way TWO workgroups per CU, whose barriers, prologues and C
// read-modify-write epilogues overlap each other's MFMA loops.
namespace vb {
constexpr int BKB = 16;
constexpr int OPER_B = BKB * LDS_LD;
constexpr int NT_B = 256;
constexpr int NQB = TILE * BKB / 2 / NT_B;  // 4

// NT form: LDS-DMA operand path.  A stage holds one chunk of BKD = 8 k of both operands, each a row-major image of 128 rows x
// 64 bytes in 16-byte (row, k pair) units, unit (x, kp) at byte 64 x + 16 (kp ^ ((x >> 2) & 3)).  An LDS-DMA writes 64 lanes x
// 16 bytes contiguously (1 KiB = 16 rows), so the swizzle goes on the global source address: lane l of a wave instruction
// fetches k pair (l & 3) ^ ((l >> 4) & 3) of row l >> 2 and lands at unit l.  A fragment read (16 consecutive rows at one k
// pair, 8 bytes per lane, two k of the pair in each 32-lane half) then covers all 64 banks once.  Four stages (64 KiB): the
// chunk c + 3 is requested at the start of chunk c and stays in flight across the barrier that ends it.
constexpr int BKD = 8;
constexpr int NSTG = 4;
constexpr int STG_OPER = TILE * BKD * 8;           // bytes of one operand's stage (8 KiB)
constexpr int STG_B = NSTG * STG_OPER;              // byte offset of B's stages
constexpr int DMA_PER_CHUNK = 2 * (STG_OPER / (NT_B * 16));  // LDS-DMA instructions per wave and chunk (A and B): 4
constexpr size_t LDS_DMA = 2 * NSTG * STG_OPER;      // 64 KiB

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(1))) void* gbl_ptr_t;

// per-lane source offset of this thread's first piece (rows 16 (4 q + wave) + (lane >> 2)) and the stride between its pieces
__device__ __forceinline__ void dma_offsets(long ld, int tid, unsigned& goff, long& gstride) {
  const int l = tid & 63, w = tid >> 6;
  const int row = 16 * w + (l >> 2), kp = (l & 3) ^ ((l >> 4) & 3);
  goff = (unsigned)((row * ld + 2 * kp) * 8);
  gstride = 64 * ld * 8;
}
// one operand's chunk into the stage at `lds_stage`: two wave instructions of 16 rows (1 KiB) each, pieces 4 q + wave
__device__ __forceinline__ void dma_chunk(const char* __restrict__ g, unsigned goff, long gstride, char* lds_stage, int wave) {
#pragma unroll
  for (int q = 0; q < 2; ++q)
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)(g + q * gstride + goff), (lds_ptr_t)(lds_stage + (4 * q + wave) * 1024), 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N == 4 || N == 16 || N == 20, "vmcnt");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
}  // namespace vb

template <bool A_KMAJOR, bool B_KMAJOR>
__global__ __launch_bounds__(vb::NT_B, 2) void gemm_f64_kernel_b(GemmParams p) {
  using vb::BKB; using vb::OPER_B; using vb::NQB;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* As = smem;               // [2][BKB][LDS_LD]
  double* Bs = smem + 2 * OPER_B;  // [2][BKB][LDS_LD]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  // XCD-aware block -> tile map for uniform-k launches (the same map stands in gemm_f64_kernel_s: keep the two in step):
  // workgroup b runs on XCD b % 8, and each XCD takes a CONTIGUOUS range of the enumeration, so the tiles of one tile row
  // (consecutive indices: they share their A rows) meet in one L2 instead of eight.
  const int nblk = gridDim.x;
  int idx = blockIdx.x;
  if (p.kmode == 0) {
    const int b = blockIdx.x, x = b & 7, q = nblk >> 3, r = nblk & 7;
    idx = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
  }
  idx += p.tile0;  // sub-range launch: the XCD-aware order above is taken inside the range
  int ti, tj;
  int rc, cc;  // C tile row / column (differ from the operand rows ti / tj only in panel-list mode)
  if (p.pl) {
    bool diag;
    list_tile(p, idx, ti, tj, rc, cc, diag);
  } else {
    // The same choice and reversal stand in gemm_f64_kernel_s (its tail form): keep the two in step.  Here the banded order
    // is taken only under the XCD-aware map (kmode 0); there kmode is always 0.
    // (full rectangles measured neutral: 8192^3 75.2 vs 75.7 TFLOP/s -- the row-major order stays for them)
    if (p.fc > 0) tile_from_index_fc(p.mt, p.nt, p.fc, p.band, idx, ti, tj);
    else if (p.band > 0 && p.tri && p.kmode == 0) tile_from_index_banded(p, idx, p.band, ti, tj);
    else tile_from_index(p, idx, ti, tj);
    // longest-k tiles first (LPT order); a triangular launch keeps its enumeration, which names only tiles on / below the diagonal
    if (p.kmode == 2 && !p.tri) ti = p.mt - 1 - ti;
    if (p.kmode == 4 && !p.tri) { tj = p.nt - 1 - idx / p.mt; ti = idx % p.mt; }
    rc = ti;
    cc = tj;
  }
  const int i0 = ti * TILE, j0 = tj * TILE;
  const KRange kr = k_range<TILE>(p, i0, j0);
  const int kbeg = kr.beg, kend = kr.end;

  const BatchPtrs bp = batch_ptrs(p);
  const double* A = bp.A;
  const double* B = bp.B;
  double* C = bp.C;

  double4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};

  const int kq = lane >> 4, l15 = lane & 15;
  double af[2][4], bf[2][4];
  // C read-modify-write: the first two of its four row groups are requested inside the last chunks of the k loop
  const double alpha = p.alpha, beta = p.beta;
  double* cbase = C + (long)(rc * TILE + wr * 64 + kq) * p.ldc + cc * TILE + wc * 64 + l15;
  double4_t cv[2][4];
  auto load_group = [&](int set, int a) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) cv[set][b][r] = cbase[(long)(16 * a + 4 * r) * p.ldc + 16 * b];
  };
  if constexpr (!A_KMAJOR && !B_KMAJOR) {
    // LDS-DMA operand path (vb::dma_offsets has the image).  Chunk c (BKD = 8 k: two k4-steps of 16 MFMAs per wave) is read from
    // stage c & 3; at its start the chunk c + 3 is requested into stage (c + 3) & 3, which chunk c - 1 has left at the last
    // barrier.  At its end each wave waits for ITS part of chunk c + 2 (a counted vmcnt: chunk c + 3 stays in flight) and the
    // barrier makes every wave's part visible; chunk c + 1's first fragments are read during chunk c's second k4-step, one
    // barrier after the wait that retired them.  The last four chunks request no operands: chunk n - 4 requests C row group 0
    // (after its DMA, so that the counts hold), chunk n - 2 row group 1.
    using vb::BKD; using vb::STG_OPER; using vb::STG_B;
    char* lds = reinterpret_cast<char*>(smem);
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    // A multiple of 4 and >= 4, which the three-chunk prologue and the four peeled last chunks rely on: k and the triangular k
    // ranges are multiples of 32 (gemm_args_error in api_blocks.hip; kseg a multiple of 128 in launch_gemm_f64).
    const int nchunk = (kend - kbeg) / BKD;
    unsigned gA, gB;
    long sA, sB;
    vb::dma_offsets(p.lda, tid, gA, sA);
    vb::dma_offsets(p.ldb, tid, gB, sB);
    const char* Ag = reinterpret_cast<const char*>(A + (long)i0 * p.lda + kbeg);
    const char* Bg = reinterpret_cast<const char*>(B + (long)j0 * p.ldb + kbeg);
    const int segmask = kseg_mask<BKD>(p);
    const long segjump = kseg_jump<BKD>(p);
    auto advance = [&](int next_chunk) {
      const long d = (next_chunk & segmask) == 0 ? segjump : (long)BKD * 8;
      Ag += d;
      Bg += d;
    };
    auto request = [&](int stg) {
      vb::dma_chunk(Ag, gA, sA, lds + stg * STG_OPER, wv);
      vb::dma_chunk(Bg, gB, sB, lds + STG_B + stg * STG_OPER, wv);
    };
    // fragment offsets of k4-steps 0 / 1: row l15 of a 16-row block, k = 4 kk + kq -> k pair 2 kk + (kq >> 1), half kq & 1
    unsigned foff[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) foff[kk] = (unsigned)(l15 * 64 + (((2 * kk + (kq >> 1)) ^ (l15 >> 2)) * 16) + (kq & 1) * 8);
    const char* a_lds = lds + wr * 64 * 64;
    const char* b_lds = lds + STG_B + wc * 64 * 64;
    auto load_frags = [&](int set, int stg, int kk) {
      const char* ap = a_lds + stg * STG_OPER + foff[kk];
      const char* bp = b_lds + stg * STG_OPER + foff[kk];
#pragma unroll
      for (int a = 0; a < 4; ++a) af[set][a] = *reinterpret_cast<const double*>(ap + 1024 * a);
#pragma unroll
      for (int b = 0; b < 4; ++b) bf[set][b] = *reinterpret_cast<const double*>(bp + 1024 * b);
    };
    request(0);
    advance(1);
    request(1);
    advance(2);
    request(2);
    advance(3);
    vb::wait_vm<vb::DMA_PER_CHUNK>();  // chunks 0 and 1
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    load_frags(0, 0, 0);
    // MODE 0: inside the loop; 1 .. 4: chunk n - 4 .. n - 1
    auto chunk_body = [&](int c, auto S, auto MODE) {
      constexpr int s = decltype(S)::value;
      constexpr int mode = decltype(MODE)::value;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        __builtin_amdgcn_sched_barrier(0);
        if (kk == 0 && mode <= 1) {
          request((s + 3) & 3);
          advance(c + 4);
        }
        if (kk == 1 && mode == 1) load_group(0, 0);
        if (kk == 0 && mode == 3) load_group(1, 1);
        if (kk == 0) load_frags(1, s, 1);
        else if (mode != 4) load_frags(0, (s + 1) & 3, 0);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[kk][a], bf[kk][b], acc[a][b], 0, 0, 0);
        if (kk == 0 && mode <= 1) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            sched_groups<SG_MFMA, 1,  SG_VMEM_READ, 1,  SG_MFMA, 1,  SG_DS_READ, 2,  SG_MFMA, 2>();
          }
        } else if (mode == 1 || (kk == 0 && mode == 3)) {
#pragma unroll
          for (int g = 0; g < 8; ++g) {
            sched_groups<SG_MFMA, 1,  SG_VMEM_READ, 2,  SG_MFMA, 1,  SG_DS_READ, 1>();
          }
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            sched_groups<SG_MFMA, 2,  SG_DS_READ, 2,  SG_MFMA, 2>();
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (mode <= 2) {
        // this wave's part of chunk c + 2 has landed (chunk c + 3 and C row group 0 may be in flight), then the barrier
        vb::wait_vm<mode == 0 ? vb::DMA_PER_CHUNK : mode == 1 ? vb::DMA_PER_CHUNK + 16 : 16>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    };
    int c = 0;
    for (; c + 4 < nchunk; c += 4) {
      chunk_body(c, std::integral_constant<int, 0>(), std::integral_constant<int, 0>());
      chunk_body(c + 1, std::integral_constant<int, 1>(), std::integral_constant<int, 0>());
      chunk_body(c + 2, std::integral_constant<int, 2>(), std::integral_constant<int, 0>());
      chunk_body(c + 3, std::integral_constant<int, 3>(), std::integral_constant<int, 0>());
    }
    chunk_body(c, std::integral_constant<int, 0>(), std::integral_constant<int, 1>());
    chunk_body(c + 1, std::integral_constant<int, 1>(), std::integral_constant<int, 2>());
    chunk_body(c + 2, std::integral_constant<int, 2>(), std::integral_constant<int, 3>());
    chunk_body(c + 3, std::integral_constant<int, 3>(), std::integral_constant<int, 4>());
  } else {
    // Even and >= 2: k and the triangular k ranges are multiples of 32 (gemm_args_error in api_blocks.hip refuses other k; the
    // library's own launches pass multiples of 128), which the prologue and the two peeled last chunks below rely on.  No
    // k-segments here: launch_gemm_f64 refuses kseg with a k-major operand.
    const int nchunk = (kend - kbeg) / BKB;
    unsigned gA, lA, gB, lB;
    long sA, sB;
    chunk_offsets<StageB, A_KMAJOR>(p.lda, tid, gA, lA, sA);
    chunk_offsets<StageB, B_KMAJOR>(p.ldb, tid, gB, lB, sB);
    const char* Ag = reinterpret_cast<const char*>(A_KMAJOR ? A + (long)kbeg * p.lda + i0 : A + (long)i0 * p.lda + kbeg);
    const char* Bg = reinterpret_cast<const char*>(B_KMAJOR ? B + (long)kbeg * p.ldb + j0 : B + (long)j0 * p.ldb + kbeg);
    const long stepA = (A_KMAJOR ? (long)BKB * p.lda : (long)BKB) * 8;
    const long stepB = (B_KMAJOR ? (long)BKB * p.ldb : (long)BKB) * 8;
    char* Asb = reinterpret_cast<char*>(As);
    char* Bsb = reinterpret_cast<char*>(Bs);
    // Global -> register prefetch runs TWO chunks ahead (register set c & 1 holds chunk c until it is written to
    // LDS buffer c & 1 during chunk c - 1): ~7k cycles of latency tolerance instead of ~3k, enough for an
    // HBM / MALL miss under load while two workgroups share the CU.
    double2_t ra[2][NQB], rb[2][NQB];
    if (nchunk > 0) {  // (always: see nchunk.  This guard and the two below stay because the k loop's registers move without them.)
      chunk_load(Ag, gA, sA, ra[0]);
      chunk_load(Bg, gB, sB, rb[0]);
      if (nchunk > 1) {
        Ag += stepA;
        Bg += stepB;
        chunk_load(Ag, gA, sA, ra[1]);
        chunk_load(Bg, gB, sB, rb[1]);
      }
      chunk_store<StageB, A_KMAJOR>(Asb, lA, ra[0]);
      chunk_store<StageB, B_KMAJOR>(Bsb, lB, rb[0]);
    }
    __syncthreads();

    const double* a_ptr = As + kq * LDS_LD + wr * 64 + l15;
    const double* b_ptr = Bs + kq * LDS_LD + wc * 64 + l15;
    auto load_frags = [&](int set, int boff, int kk) {
      const double* ap = a_ptr + boff + kk * 4 * LDS_LD;
      const double* bp = b_ptr + boff + kk * 4 * LDS_LD;
  #pragma unroll
      for (int a = 0; a < 4; ++a) af[set][a] = ap[16 * a];
  #pragma unroll
      for (int b = 0; b < 4; ++b) bf[set][b] = bp[16 * b];
    };
    if (nchunk > 0) load_frags(0, 0, 0);

    // one chunk; S = c & 1 selects both the LDS buffer being consumed and the register set being refilled.
    // The body is branch-free (loads / stores of the last chunks are redundant instead of skipped) so that it is
    // one scheduling region, and sched_group_barrier spreads the memory instructions between the 64 MFMAs:
    //   k4-step 0: 8 global loads (chunk c+2) + the 4 ds_read2 of step 1     step 1, 2: the 4 ds_read2 of the next step
    //   k4-step 3: the 8 ds_write2 of chunk c+1
    // A burst of LDS / VMEM issue in both co-resident workgroups at once left the MFMA pipe 88 % busy; spread out
    // it is 93 % (8192^3: 70.3 -> 73.3 TFLOP/s, rocBLAS 72.9).
    // C row groups 0 and 1 are requested during the LAST two chunks of the k loop (in place of those chunks' global prefetches,
    // which would be redundant reloads), so that their round trip hides under 128 MFMAs instead of following the loop
    auto chunk_body = [&](int c, auto S, auto LASTC) {
      constexpr int s = decltype(S)::value;
      constexpr int lastc = decltype(LASTC)::value;  // 0: inside the loop; 1 / 2: second-to-last / last chunk
      constexpr int boff = s * OPER_B;
      const bool adv = (c + 2 < nchunk);
      Ag += adv ? stepA : 0;
      Bg += adv ? stepB : 0;
  #pragma unroll
      for (int kk = 0; kk < BKB / 4; ++kk) {
        const int cur = kk & 1;
        __builtin_amdgcn_sched_barrier(0);
        if (kk == 0) {
          if (lastc == 0) {
            chunk_load(Ag, gA, sA, ra[s]);
            chunk_load(Bg, gB, sB, rb[s]);
          } else {
            load_group(lastc - 1, lastc - 1);
          }
        }
        if (kk + 1 < BKB / 4) load_frags(cur ^ 1, boff, kk + 1);
  #pragma unroll
        for (int a = 0; a < 4; ++a)
  #pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[cur][a], bf[cur][b], acc[a][b], 0, 0, 0);
        if (kk == BKB / 4 - 1) {
          constexpr int noff = (boff ^ OPER_B) * 8;
          chunk_store<StageB, A_KMAJOR>(Asb + noff, lA, ra[s ^ 1]);
          chunk_store<StageB, B_KMAJOR>(Bsb + noff, lB, rb[s ^ 1]);
        }
        if (kk == 0) {
  #pragma unroll
          for (int g = 0; g < 4; ++g) {
            sched_groups<SG_MFMA, 1,  SG_VMEM_READ, 1,  SG_MFMA, 1,  SG_VMEM_READ, 1,  SG_MFMA, 1,  SG_DS_READ, 1,  SG_MFMA, 1>();
          }
        } else if (kk + 1 < BKB / 4) {
  #pragma unroll
          for (int g = 0; g < 4; ++g) {
            sched_groups<SG_MFMA, 3,  SG_DS_READ, 1,  SG_MFMA, 1>();
          }
        } else {
          constexpr int nw = (A_KMAJOR ? NQB : 2 * NQB) + (B_KMAJOR ? NQB : 2 * NQB);  // ds_write instructions
  #pragma unroll
          for (int g = 0; g < 16; ++g) {
            sched_groups<SG_MFMA, 1>();
            if (g < nw) sched_groups<SG_DS_WRITE, 1>();
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();
      load_frags(0, boff ^ OPER_B, 0);
    };
    int c = 0;
    for (; c + 2 < nchunk; c += 2) {
      chunk_body(c, std::integral_constant<int, 0>(), std::integral_constant<int, 0>());
      chunk_body(c + 1, std::integral_constant<int, 1>(), std::integral_constant<int, 0>());
    }
    chunk_body(c, std::integral_constant<int, 0>(), std::integral_constant<int, 1>());
    chunk_body(c + 1, std::integral_constant<int, 1>(), std::integral_constant<int, 2>());
  }

  if (beta != 0.0) {
    // row groups 0 and 1 are in registers; groups 2 and 3 are requested while 0 and 1 are stored
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          cbase[(long)(16 * a + 4 * r) * p.ldc + 16 * b] = alpha * acc[a][b][r] + beta * cv[a & 1][b][r];
      if (a + 2 < 4) load_group(a & 1, a + 2);
    }
  } else {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) cbase[(long)(16 * a + 4 * r) * p.ldc + 16 * b] = alpha * acc[a][b][r];
  }
}

// ---------------------------------------------------------------------------------------------
// 64x64 tiles: 64x64 output tile per 256-thread workgroup (4 waves as 2x2, 32x32 per wave) for launches
// with too few 128x128 tiles to fill the chip (the in-panel updates of the Cholesky, a few dozen to a
// few hundred tiles, which sit on the factorisation's critical path): 4x the workgroups, 1/4 of the
// per-workgroup latency.  GemmParams.mt / nt are reinterpreted in 64-row tiles by the launcher.
namespace vs {
constexpr int TS = StageS::T;
constexpr int BKS = 16;
constexpr int LDS_S = StageS::LD;
constexpr int OPER_S = BKS * LDS_S;
constexpr int NQS = TS * BKS / 2 / 256;  // 2
constexpr int NBUF = 3;                  // LDS buffers per operand (see the pipeline note in the kernel)

}  // namespace vs

// FLUSH: the k-segmented update (GemmParams::kflush) -- an instantiation of its own, so that the plain kernel keeps the code
// and the registers it was tuned with (the flush as a run-time branch cost every launch 4 %: N = 16384 25.0 -> 25.9 ms)
template <bool A_KMAJOR, bool B_KMAJOR, bool FLUSH = false>
__global__ __launch_bounds__(256, 2) void gemm_f64_kernel_s(GemmParams p) {
  using vs::BKS; using vs::OPER_S; using vs::NQS; using vs::LDS_S; using vs::TS;
  if (p.hiprio) __builtin_amdgcn_s_setprio(3);  // panel-chain launches: win the SIMD's issue arbitration against bulk waves
  __shared__ __attribute__((aligned(16))) double smem[2 * vs::NBUF * vs::OPER_S];
  double* As = smem;
  double* Bs = smem + vs::NBUF * OPER_S;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  int ti, tj;
  int rc, cc;  // C tile row / column in 64-row units (differ from the operand rows ti / tj only in panel-list mode)
  // XCD-aware block -> tile map for uniform-k launches: the map of gemm_f64_kernel_b, which explains it (keep the two in
  // step); no tile0 here, small launches are never split
  int bid = (int)blockIdx.x;
  if (p.kmode == 0) {
    const int nblk = (int)gridDim.x, x = bid & 7, q = nblk >> 3, r = nblk & 7;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
  }
  if (p.pl) {
    // panel-list launch (or the tail of one): this workgroup is one quadrant of 128x128 tile sub_base + bid / 4
    int ra, rb, prc, pcc;
    bool diag;
    const int quad = bid & 3;
    list_tile(p, p.sub_base + (bid >> 2), ra, rb, prc, pcc, diag);
    if (diag && quad == 1) return;  // the quadrant above the diagonal of a diagonal tile
    ti = 2 * ra + (quad >> 1);
    tj = 2 * rb + (quad & 1);
    rc = 2 * prc + (quad >> 1);
    cc = 2 * pcc + (quad & 1);
  } else {
    if (p.sub_base >= 0) {
      // tail of a 128x128-tile launch: this workgroup is one quadrant of parent tile sub_base + blockIdx.x / 4
      int pti, ptj;
      const int pidx = p.sub_base + (bid >> 2), quad = bid & 3;
      // the parent launch's order, as gemm_f64_kernel_b chooses it (keep the two in step; tails are uniform-k, kmode is 0 here)
      if (p.fc > 0) tile_from_index_fc(p.sub_mt, p.sub_nt, p.fc, p.band, pidx, pti, ptj);
      else if (p.band > 0 && p.tri) tile_from_index_banded(p.tri, p.sub_mt, p.sub_nt, pidx, p.band, pti, ptj);
      else tile_from_index(p.tri, p.sub_nt, pidx, pti, ptj);
      ti = 2 * pti + (quad >> 1);
      tj = 2 * ptj + (quad & 1);
      if (p.tri && tj > ti) return;  // the quadrant above the diagonal of a diagonal parent tile
      if (p.dead_last_half && ti == 2 * p.sub_mt - 1) return;  // the all-zero half of the y^T tile row
    } else {
      tile_from_index(p, bid, ti, tj);  // a whole launch on 64x64 tiles: row by row only, never fc or banded
      if (p.dead_last_half && ti == p.mt - 1) return;
    }
    // longest-k tiles first, as in gemm_f64_kernel_b (keep the two in step; kmode is not 0 here, so bid is blockIdx.x)
    if (p.kmode == 2 && !p.tri) ti = p.mt - 1 - ti;
    if (p.kmode == 4 && !p.tri) { tj = p.nt - 1 - (int)blockIdx.x / p.mt; ti = (int)blockIdx.x % p.mt; }
    rc = ti;
    cc = tj;
  }
  const int i0 = ti * TS, j0 = tj * TS;
  const KRange kr = k_range<TS>(p, i0, j0);
  const int kbeg = kr.beg & ~(BKS - 1), kend = kr.end;  // this kernel rounds the start down to a whole chunk

  const BatchPtrs bp = batch_ptrs(p);
  const double* A = bp.A;
  const double* B = bp.B;
  double* C = bp.C;

  double4_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};

  const int nchunk = (kend - kbeg) / BKS;
  unsigned gA, lA, gB, lB;
  long sA, sB;
  chunk_offsets<StageS, A_KMAJOR>(p.lda, tid, gA, lA, sA);
  chunk_offsets<StageS, B_KMAJOR>(p.ldb, tid, gB, lB, sB);
  const char* Ag = reinterpret_cast<const char*>(A_KMAJOR ? A + (long)kbeg * p.lda + i0 : A + (long)i0 * p.lda + kbeg);
  const char* Bg = reinterpret_cast<const char*>(B_KMAJOR ? B + (long)kbeg * p.ldb + j0 : B + (long)j0 * p.ldb + kbeg);
  const long stepA = (A_KMAJOR ? (long)BKS * p.lda : (long)BKS) * 8;
  const long stepB = (B_KMAJOR ? (long)BKS * p.ldb : (long)BKS) * 8;
  const int segmask = kseg_mask<BKS>(p);
  const long segjump = kseg_jump<BKS>(p);
  char* Asb = reinterpret_cast<char*>(As);
  char* Bsb = reinterpret_cast<char*>(Bs);
  // Pipeline (chunk = 16 k = 16 MFMAs per wave, 0.43 us): chunk c is requested from global memory during chunk c - 4
  // (one-chunk prefetch, round 1: every chunk waited for its load, 1.4 us per chunk), parked in register set c % 3,
  // written to LDS buffer c % 3 at the end of chunk c - 2, and its first operand fragments are read during the last
  // k-step of chunk c - 1 -- BEFORE that chunk's barrier, which is possible because the buffer became visible one barrier
  // earlier.  With two LDS buffers the fragment read followed the barrier and every chunk began with an LDS round trip
  // (~150 cycles of 1024 + 150); the third buffer costs 20 KB (60 KB per workgroup, two workgroups per CU still fit).
  constexpr int NB = vs::NBUF;  // 3
  double2_t ra[NB][NQS], rb[NB][NQS];
  auto advance = [&](int next_chunk) {  // chunks beyond the last are redundant reloads of the last one, never consumed
    const bool adv = next_chunk < nchunk;
    const bool seg = (next_chunk & segmask) == 0;
    Ag += adv ? (seg ? segjump : stepA) : 0;
    Bg += adv ? (seg ? segjump : stepB) : 0;
  };
  if (nchunk > 0) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      chunk_load(Ag, gA, sA, ra[u]);
      chunk_load(Bg, gB, sB, rb[u]);
      advance(u + 1);
    }
    chunk_store<StageS, A_KMAJOR>(Asb, lA, ra[0]);
    chunk_store<StageS, B_KMAJOR>(Bsb, lB, rb[0]);
    chunk_store<StageS, A_KMAJOR>(Asb + OPER_S * 8, lA, ra[1]);
    chunk_store<StageS, B_KMAJOR>(Bsb + OPER_S * 8, lB, rb[1]);
    chunk_load(Ag, gA, sA, ra[0]);  // chunk 3
    chunk_load(Bg, gB, sB, rb[0]);
    advance(4);
  }
  // C tile early: these launches are latency-bound, the read hides under the whole k loop
  const int kq = lane >> 4, l15 = lane & 15;
  const double alpha = p.alpha, beta = p.beta;
  double* cbase = C + (long)(rc * TS + wr * 32 + kq) * p.ldc + cc * TS + wc * 32 + l15;
  double4_t cv[2][2];
  if (beta != 0.0) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) cv[a][b][r] = cbase[(long)(16 * a + 4 * r) * p.ldc + 16 * b];
  }
  __syncthreads();

  // fragment bases per k4-step: the row-major operands' images are swizzled by the k pair (chunk_offsets, StageS), k & 14 =
  // 4 kk + (kq & 2) for k = 4 kk + kq
  const double* a_ptr[4];
  const double* b_ptr[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int sa = !A_KMAJOR ? (4 * kk + (kq & 2)) : 0, sb = !B_KMAJOR ? (4 * kk + (kq & 2)) : 0;
    a_ptr[kk] = As + kq * LDS_S + wr * 32 + (l15 ^ sa);
    b_ptr[kk] = Bs + kq * LDS_S + wc * 32 + (l15 ^ sb);
  }
  // Same schedule as the 128x128 kernel at a quarter of the tile: branch-free chunk body, operand fragments double-buffered
  // one k4-step ahead, and the chunk's 4 global loads / 8 fragment reads / LDS writes spread between its 16 MFMAs.
  double fa[2][2], fb[2][2];
  auto load_frags = [&](int set, int boff, int kk) {
    const double* ap = a_ptr[kk] + boff + kk * 4 * LDS_S;
    const double* bp = b_ptr[kk] + boff + kk * 4 * LDS_S;
    fa[set][0] = ap[0]; fa[set][1] = ap[16]; fb[set][0] = bp[0]; fb[set][1] = bp[16];
  };
  if (nchunk > 0) load_frags(0, 0, 0);
  // one chunk c; S = c % 3: LDS buffer consumed; register set (S + 1) % 3 is refilled with chunk c + 4; register set and
  // LDS buffer (S + 2) % 3 take part in the hand-over of chunk c + 2
  const int kflush_chunks = FLUSH ? p.kflush / BKS : 1;
  auto chunk_body = [&](int c, auto Sc) {
    constexpr int sidx = decltype(Sc)::value;
    constexpr int boff = sidx * OPER_S;
    constexpr int s1 = (sidx + 1) % NB, s2 = (sidx + 2) % NB;
#pragma unroll
    for (int kk = 0; kk < BKS / 4; ++kk) {
      const int cur = kk & 1;
      __builtin_amdgcn_sched_barrier(0);
      if (kk == 0) {
        chunk_load(Ag, gA, sA, ra[s1]);
        chunk_load(Bg, gB, sB, rb[s1]);
      }
      if (kk + 1 < BKS / 4) load_frags(cur ^ 1, boff, kk + 1);
      else load_frags(cur ^ 1, s1 * OPER_S, 0);  // first fragments of the next chunk, ahead of the barrier
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][0], fb[cur][0], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][0], fb[cur][1], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][1], fb[cur][0], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[cur][1], fb[cur][1], acc[1][1], 0, 0, 0);
      if (kk == BKS / 4 - 1) {
        chunk_store<StageS, A_KMAJOR>(Asb + s2 * OPER_S * 8, lA, ra[s2]);
        chunk_store<StageS, B_KMAJOR>(Bsb + s2 * OPER_S * 8, lB, rb[s2]);
      }
      if (kk == 0) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          sched_groups<SG_MFMA, 1,  SG_VMEM_READ, 1,  SG_DS_READ, 1,  SG_MFMA, 1,  SG_VMEM_READ, 1>();
        }
      } else if (kk + 1 < BKS / 4) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          sched_groups<SG_MFMA, 1,  SG_DS_READ, 1,  SG_MFMA, 1>();
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          sched_groups<SG_MFMA, 1,  SG_DS_READ, 1,  SG_DS_WRITE, 2>();
        }
      }
    }
    advance(c + 5);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (FLUSH) if ((c + 1) % kflush_chunks == 0 && c + 1 < nchunk) {
      // k-segmented update (GemmParams::kflush): C takes this segment's sum NOW, rounded as a launch of its own would round
      // it, and the accumulators start the next segment at zero -- one launch then returns the bits of one launch per segment
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double v = alpha * acc[a][b][r];
            v += beta * cv[a][b][r];
            cv[a][b][r] = v;
          }
          acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
        }
    }
    __syncthreads();
  };
  int c = 0;
  for (; c + 3 <= nchunk; c += 3) {
    chunk_body(c, std::integral_constant<int, 0>());
    chunk_body(c + 1, std::integral_constant<int, 1>());
    chunk_body(c + 2, std::integral_constant<int, 2>());
  }
  if (c < nchunk) chunk_body(c, std::integral_constant<int, 0>());  // c is a multiple of 3 here
  if (c + 1 < nchunk) chunk_body(c + 1, std::integral_constant<int, 1>());
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double v = alpha * acc[a][b][r];
        if (beta != 0.0) v += beta * cv[a][b][r];
        cbase[(long)(16 * a + 4 * r) * p.ldc + 16 * b] = v;
      }
}


// Every instantiation, once: the launcher looks its kernel up here and gemm_f64_enable_lds walks the whole table.
typedef void (*gemm_kernel_t)(GemmParams);
struct GemmKernel { gemm_kernel_t fn; bool small, flush; int a_kmajor, b_kmajor; };  // small: 64x64 tiles; flush: GemmParams::kflush
static const GemmKernel GEMM_KERNELS[] = {
    {gemm_f64_kernel_b<false, false>, false, false, 0, 0}, {gemm_f64_kernel_b<false, true>, false, false, 0, 1},
    {gemm_f64_kernel_b<true, false>, false, false, 1, 0},  {gemm_f64_kernel_b<true, true>, false, false, 1, 1},
    {gemm_f64_kernel_s<false, false>, true, false, 0, 0},  {gemm_f64_kernel_s<false, true>, true, false, 0, 1},
    {gemm_f64_kernel_s<true, false>, true, false, 1, 0},   {gemm_f64_kernel_s<true, true>, true, false, 1, 1},
    {gemm_f64_kernel_s<false, false, true>, true, true, 0, 0},
};
static gemm_kernel_t gemm_kernel(bool small, bool flush, int a_kmajor, int b_kmajor) {
  for (const GemmKernel& k : GEMM_KERNELS)
    if (k.small == small && k.flush == flush && k.a_kmajor == !!a_kmajor && k.b_kmajor == !!b_kmajor) return k.fn;
  return nullptr;  // (only the NT form has a flush instantiation; launch_gemm_f64 refuses the others before it asks)
}

constexpr size_t LDS_ONE_PER_CU = 82432;  // > half a CU (one workgroup per CU) and <= 160 KB - the 79 KB leaf image

static int tile_count(const GemmParams& p) {
  if (p.pl) return p.pl_tiles;
  if (!p.tri) return p.mt * p.nt;
  return p.nt * (p.nt + 1) / 2 + (p.mt - p.nt) * p.nt;
}


// launches with fewer 128x128 tiles than p.small_below run on 64x64 tiles (4x the workgroups, 1/4 of the latency)
bool gemm_uses_small_tiles(const GemmParams& p, int batch) {
  if (p.kflush > 0) return true;  // (the 64x64-tile kernel holds its C tile in registers from the start: only it can flush per k-segment)
  return tile_count(p) * batch < p.small_below && p.kmode != 2;
}

// The 128x128-tile kernel runs its tiles in rounds of 512 (two workgroups on each of 256 CUs, 218 us per round at
// k = 1024): a last round with few tiles costs a whole round (7 % of the nine bulk launches of an N = 16384
// factorisation).  Uniform-k launches therefore hand the tiles beyond the last full round to the 64x64-tile kernel (a
// quarter of the time per round): worth it up to 384 such tiles (three quarter-rounds).  The rule does not look at
// one_per_cu or the stream, so results stay bit-identical across the scheduling options.
constexpr int ROUND_TILES = 512, TAIL_MAX_TILES = 384;
constexpr int NARROW_TRAPEZOID_COLS = 8;
int gemm_tail_tiles(const GemmParams& p, int batch) {
  if (!p.tail_small || p.kmode != 0 || batch != 1 || gemm_uses_small_tiles(p, batch)) return 0;
  const int nblk = tile_count(p), rem = nblk % ROUND_TILES;
  return (nblk > ROUND_TILES && rem > 0 && rem <= TAIL_MAX_TILES) ? rem : 0;
}

hipError_t launch_gemm_f64(const GemmParams& p_in, int opA_kmajor, int opB_kmajor, int batch, hipStream_t stream, int part) {
  GemmParams p = p_in;
  // Narrow trapezoids (the next-panel and in-panel updates: at most 8 tile columns under a tall panel) keep the row-major
  // order: a tile row's <= 8 tiles share one 1 MB row strip of A and the column strips (<= 8 MB) are common to all rows,
  // while bands of 8 rows x 8 columns touch 16 MB per 64 tiles (15360 x 1024, k = 1024 on 128x128 tiles: 545 vs 558 us;
  // 8192 x 1024: 253 vs 264 us).  Wide trapezoids (the bulk updates) keep the band-column-major order of section 5.1.
  if (p.tri && !p.pl && p.nt <= NARROW_TRAPEZOID_COLS) p.band = 0;
  if (!(p.tri && !p.pl && p.kmode == 0 && p.fc > 0 && p.fc < p.nt)) p.fc = 0;
  if (p.kseg != 0 && (p.kseg < 0 || p.kseg % 128 || p.kmode != 0 || opA_kmajor || opB_kmajor || p.k % p.kseg))
    return hipErrorInvalidValue;  // k-segments: whole tile columns, the NT form, uniform k
  const int nblk = tile_count(p);
  if (nblk <= 0 || batch <= 0) return hipSuccess;
  const bool small = gemm_uses_small_tiles(p, batch);
  const int tail = gemm_tail_tiles(p, batch);
  // 64x64 tiles: the whole product (few 128x128 tiles: same enumeration, tile units halve) or the `ntail` last tiles of
  // a 128x128-tile launch
  auto launch_small = [&](int ntail) -> hipError_t {
    GemmParams q = p;
    q.mt = 2 * p.mt;
    q.nt = 2 * p.nt;
    int nwg = tile_count(q);
    if (ntail > 0) {
      q.sub_base = nblk - ntail;
      q.sub_mt = p.mt;
      q.sub_nt = p.nt;
      nwg = 4 * ntail;
    } else if (p.pl) {  // a whole panel-list launch on 64x64 tiles: four quadrant workgroups per 128x128 tile
      q.sub_base = 0;
      nwg = 4 * nblk;
    }
    dim3 grid(nwg, 1, batch), block(256);
    // one_per_cu: unused dynamic LDS on top of the 60 KB static image pushes the request over half a CU
    const size_t pad = p.one_per_cu ? LDS_ONE_PER_CU - sizeof(double) * 2 * vs::NBUF * vs::OPER_S : 0;
    if (q.kflush > 0 && (opA_kmajor || opB_kmajor || q.kmode != 0 || q.beta == 0.0 || q.kflush % vs::BKS)) return hipErrorInvalidValue;
    gemm_kernel(true, q.kflush > 0, opA_kmajor, opB_kmajor)<<<grid, block, pad, stream>>>(q);
    return hipGetLastError();
  };
  if (small) return (part == 2 || p.tile0 > 0) ? hipSuccess : launch_small(0);  // small launches are never split
  // sub-range [t0, t1) of the enumeration: the 128x128-tile kernel takes what lies in front of the tail, the tail goes
  // with the range that reaches the end
  const int t0 = p.tile0, t1 = p.tile_cnt > 0 ? (t0 + p.tile_cnt < nblk ? t0 + p.tile_cnt : nblk) : nblk;
  const int big_end = t1 < nblk - tail ? t1 : nblk - tail;
  if (part != 2 && big_end > t0) {
    dim3 grid(big_end - t0, 1, batch), block(vb::NT_B);
    const bool dma = !opA_kmajor && !opB_kmajor;  // the NT form stages its operands by LDS-DMA (64 KiB), the others by registers
    const size_t lds = p.one_per_cu ? LDS_ONE_PER_CU : dma ? vb::LDS_DMA : sizeof(double) * 4 * vb::OPER_B;
    gemm_kernel(false, false, opA_kmajor, opB_kmajor)<<<grid, block, lds, stream>>>(p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return (tail > 0 && part != 1 && t1 == nblk) ? launch_small(tail) : hipSuccess;
}

hipError_t gemm_f64_enable_lds() {
  for (const GemmKernel& k : GEMM_KERNELS) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_ONE_PER_CU);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace migp
