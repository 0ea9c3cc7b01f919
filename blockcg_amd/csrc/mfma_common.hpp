// Shared device helpers of the MFMA fast path (kernels_mfma.hip: the row kernels; kernels_stencil.hip: the stencil):
// the MFMA wrappers, coefficient matrices in LDS, the 16-row tile and its products, Gram accumulation and the in-kernel
// fold of Gram partials.  Everything lives in an anonymous namespace: each translation unit has its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "kernels_mfma.hpp"

#include <type_traits>

namespace bcg {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double dv2 __attribute__((ext_vector_type(2)));  // native vector: promotes to registers where HIP's double2 struct does not

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ d4 mfma_nega(double a, double b, d4 c) {  // c + (-a) * b
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 1);
}

__device__ __forceinline__ double2 ld_nt(const double2* p) {
  const dv2 v = __builtin_nontemporal_load(reinterpret_cast<const dv2*>(p));
  return make_double2(v.x, v.y);
}
// write-through store (sc1): visible device-wide without a release fence -- the hand-off of Gram partials to the folding block
__device__ __forceinline__ void st_sc1(double2* p, double2 v) {
  dv2 w;
  w.x = v.x;
  w.y = v.y;
  asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(w));
}

// ---- coefficient matrices in LDS ------------------------------------------------------------------
// Layout: Ml[j_in * LD + 2*j_out + comp], LD = 2M + 1 doubles (row stride M*16 + 8 bytes keeps the
// two 16-lane halves of a ds_read_b64 group on disjoint banks).
template <int M>
struct MatLds {
  static constexpr int LD = 2 * M + 1;
  static constexpr int DOUBLES = M * LD;
};

// global: complex column-major, element (i,j) at j*M + i.
template <int M>
__device__ __forceinline__ void stage_matrix(double* Ml, const double2* __restrict__ Cg, int tid, int nthreads) {
  for (int e = tid; e < M * M; e += nthreads) {
    const int i = e % M, jo = e / M;
    const double2 v = Cg[e];
    Ml[i * MatLds<M>::LD + 2 * jo] = v.x;
    Ml[i * MatLds<M>::LD + 2 * jo + 1] = v.y;
  }
}

// ---- 16-row tile in (r = l&15, kq = l>>4) ownership -------------------------------------------------
template <int M>
struct Tile {
  double2 v[M / 4];
};

// ok: this lane's row exists.  Callers pass a wave-uniform `true` for every tile but the field's last one when the row count
// is no multiple of 16 (BCG_ROWS_FULL below): the loads and stores of a full tile are then straight-line code instead of
// one predicated block per instruction.
template <int M>
__device__ __forceinline__ void tile_load(Tile<M>& t, const double2* __restrict__ f, int64_t row, int kq, bool ok) {
  const double2* p = f + row * M + kq;
#pragma unroll
  for (int s = 0; s < M / 4; ++s) t.v[s] = ok ? p[4 * s] : make_double2(0.0, 0.0);
}
template <int M>
__device__ __forceinline__ void tile_store(const Tile<M>& t, double2* __restrict__ f, int64_t row, int kq, bool ok) {
  double2* p = f + row * M + kq;
  if (ok) {
#pragma unroll
    for (int s = 0; s < M / 4; ++s) p[4 * s] = t.v[s];
  }
}
#ifdef BCG_ROWS_ALWAYS_FULL  // timing build: valid only for row counts that are multiples of 16
#define BCG_ROW_OK(row, rows) true
#else
#define BCG_ROW_OK(row, rows) ((row) < (rows))
#endif


// accumulator fragments <-> tile.  Output element (s_o, ri_o) of the lane sits in acc[q>>2][q&3],
// q = ri_o*(M/4) + s_o.
template <int M>
struct Acc {
  d4 a[M / 8];
};
template <int M>
__device__ __forceinline__ void acc_from_tile(Acc<M>& A, const Tile<M>& t) {
#pragma unroll
  for (int s = 0; s < M / 4; ++s) {
    A.a[s >> 2][s & 3] = t.v[s].x;
    A.a[(M / 4 + s) >> 2][(M / 4 + s) & 3] = t.v[s].y;
  }
}
template <int M>
__device__ __forceinline__ void acc_zero(Acc<M>& A) {
#pragma unroll
  for (int q = 0; q < M / 8; ++q) A.a[q] = d4{0.0, 0.0, 0.0, 0.0};
}
template <int M>
__device__ __forceinline__ void tile_from_acc(Tile<M>& t, const Acc<M>& A) {
#pragma unroll
  for (int s = 0; s < M / 4; ++s) {
    t.v[s].x = A.a[s >> 2][s & 3];
    t.v[s].y = A.a[(M / 4 + s) >> 2][(M / 4 + s) & 3];
  }
}

// acc += in * C   (C staged in LDS at Ml).  For M >= 16 the re/im block of an output tile is the same for all
// lanes, so the choice between Re C and Im C and the sign are compile-time (the minus is the MFMA's NEG modifier).
// For M = 8 one 16 x 16 tile holds both blocks: the A-operand lane picks its coefficient by its own output slot.
//
// Three real products instead of four (Gauss) where kGauss3M<M>: with x = in, c = Re C, d = Im C,
//   K = (x_re + x_im) c ,  out_re = acc_re - x_im (c + d) + K ,  out_im = acc_im + x_re (d - c) + K.
// The re and im accumulators run their chains from acc, K from zero; K is added at the end of the same call.  Every
// rounding of a call depends on (acc, in, C) only, and rmul_acc2 runs this chain for each of its accumulators, so the
// bit-identities between the fused kernels and the plain ones hold as in the four-product form.  The sums c + d, d - c
// and x_re + x_im are formed per k-step from the values the lane reads anyway (the LDS layout is the same).
// M = 8: one 16 x 16 tile holds both blocks and three products save nothing.  M = 32: not switched (kept at four
// products).  -DBCG_COMPLEX_4M builds the four-product form everywhere (A/B builds).
#ifdef BCG_COMPLEX_4M
template <int M>
constexpr bool kGauss3M = false;
#else
template <int M>
constexpr bool kGauss3M = M == 16;
#endif

// The end of a Gauss product: K added to the re block (AR) and the im block (AI) of one output half.
__device__ __forceinline__ void rmul_gauss_fold(d4& AR, d4& AI, const d4& K) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    AR[i] += K[i];
    AI[i] += K[i];
  }
}

template <int M>
__device__ __forceinline__ void rmul_acc(Acc<M>& A, const Tile<M>& in, const double* Ml, int lane) {
  static_assert(M == 8 || M == 16 || M == 32, "MFMA right-multiply is instantiated for m = 8, 16, 32");
  constexpr int LD = MatLds<M>::LD;
  const int kq = lane >> 4;          // which of the 4 k-slots of a step this lane feeds (B operand)
  const int ar = lane & 15;          // A-operand row: output slot dr = kq_o + 4*reg_o
  if constexpr (kGauss3M<M>) {
    constexpr int H = M / 16;        // output halves: A.a[h] is the re block of half h, A.a[H + h] its im block
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int j_o = 4 * (4 * h + (ar >> 2)) + (ar & 3);
      const double* base = Ml + kq * LD + 2 * j_o;
      d4 K = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s_i = 0; s_i < M / 4; ++s_i) {
        const double c = base[s_i * 4 * LD + 0];                 // Re C(j_i, j_o)
        const double d = base[s_i * 4 * LD + 1];                 // Im C(j_i, j_o)
        K = mfma(c, in.v[s_i].x + in.v[s_i].y, K);
        A.a[h] = mfma_nega(c + d, in.v[s_i].y, A.a[h]);
        A.a[H + h] = mfma(d - c, in.v[s_i].x, A.a[H + h]);
      }
      rmul_gauss_fold(A.a[h], A.a[H + h], K);
    }
    return;
  }
#pragma unroll
  for (int T = 0; T < (M + 7) / 8; ++T) {
    const int q_o = 4 * T + (ar >> 2);                           // output slot index: ri_o*(M/4) + s_o
    const int ri_o = q_o / (M / 4);                              // lane independent for M >= 16
    const int s_o = q_o % (M / 4);
    const int j_o = 4 * s_o + (ar & 3);
    const double* base = Ml + kq * LD + 2 * j_o;                 // + s_i*4*LD + comp
#pragma unroll
    for (int s_i = 0; s_i < M / 4; ++s_i) {
      const double a_same = base[s_i * 4 * LD + 0];              // Re C(j_i, j_o)
      const double a_cross = base[s_i * 4 * LD + 1];             // Im C(j_i, j_o)
      if (M >= 16) {
        if ((4 * T) / (M / 4) == 0) {
          // out_re += in_re * Re C - in_im * Im C
          A.a[T] = mfma(a_same, in.v[s_i].x, A.a[T]);
          A.a[T] = mfma_nega(a_cross, in.v[s_i].y, A.a[T]);
        } else {
          // out_im += in_re * Im C + in_im * Re C
          A.a[T] = mfma(a_cross, in.v[s_i].x, A.a[T]);
          A.a[T] = mfma(a_same, in.v[s_i].y, A.a[T]);
        }
      } else {
        const double c_re = ri_o ? a_cross : a_same;             // coefficient of in_re for this lane's output slot
        const double c_im = ri_o ? a_same : -a_cross;            // coefficient of in_im
        A.a[T] = mfma(c_re, in.v[s_i].x, A.a[T]);
        A.a[T] = mfma(c_im, in.v[s_i].y, A.a[T]);
      }
    }
  }
}

// Two products sharing the B operand (the P_s tile): X += P*Ca and Pn += P*Cb.
template <int M>
__device__ __forceinline__ void rmul_acc2(Acc<M>& A1, const double* Ml1, Acc<M>& A2, const double* Ml2, const Tile<M>& in,
                                          int lane) {
  constexpr int LD = MatLds<M>::LD;
  const int kq = lane >> 4;
  const int ar = lane & 15;
  if constexpr (kGauss3M<M>) {  // rmul_acc's chain for each accumulator; the B operands and x_re + x_im are shared
    constexpr int H = M / 16;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int off = kq * LD + 2 * (4 * (4 * h + (ar >> 2)) + (ar & 3));
      d4 K1 = d4{0.0, 0.0, 0.0, 0.0}, K2 = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s_i = 0; s_i < M / 4; ++s_i) {
        const double c1 = Ml1[off + s_i * 4 * LD], d1 = Ml1[off + s_i * 4 * LD + 1];
        const double c2 = Ml2[off + s_i * 4 * LD], d2 = Ml2[off + s_i * 4 * LD + 1];
        const double xs = in.v[s_i].x + in.v[s_i].y;
        K1 = mfma(c1, xs, K1);
        K2 = mfma(c2, xs, K2);
        A1.a[h] = mfma_nega(c1 + d1, in.v[s_i].y, A1.a[h]);
        A2.a[h] = mfma_nega(c2 + d2, in.v[s_i].y, A2.a[h]);
        A1.a[H + h] = mfma(d1 - c1, in.v[s_i].x, A1.a[H + h]);
        A2.a[H + h] = mfma(d2 - c2, in.v[s_i].x, A2.a[H + h]);
      }
      rmul_gauss_fold(A1.a[h], A1.a[H + h], K1);
      rmul_gauss_fold(A2.a[h], A2.a[H + h], K2);
    }
    return;
  }
#pragma unroll
  for (int T = 0; T < (M + 7) / 8; ++T) {
    const int q_o = 4 * T + (ar >> 2);
    const int ri_o = q_o / (M / 4);
    const int s_o = q_o % (M / 4);
    const int j_o = 4 * s_o + (ar & 3);
    const int off = kq * LD + 2 * j_o;
#pragma unroll
    for (int s_i = 0; s_i < M / 4; ++s_i) {
      const double a1s = Ml1[off + s_i * 4 * LD], a1c = Ml1[off + s_i * 4 * LD + 1];
      const double a2s = Ml2[off + s_i * 4 * LD], a2c = Ml2[off + s_i * 4 * LD + 1];
      if (M >= 16) {
        if ((4 * T) / (M / 4) == 0) {
          A1.a[T] = mfma(a1s, in.v[s_i].x, A1.a[T]);
          A2.a[T] = mfma(a2s, in.v[s_i].x, A2.a[T]);
          A1.a[T] = mfma_nega(a1c, in.v[s_i].y, A1.a[T]);
          A2.a[T] = mfma_nega(a2c, in.v[s_i].y, A2.a[T]);
        } else {
          A1.a[T] = mfma(a1c, in.v[s_i].x, A1.a[T]);
          A2.a[T] = mfma(a2c, in.v[s_i].x, A2.a[T]);
          A1.a[T] = mfma(a1s, in.v[s_i].y, A1.a[T]);
          A2.a[T] = mfma(a2s, in.v[s_i].y, A2.a[T]);
        }
      } else {
        const double c1r = ri_o ? a1c : a1s, c1i = ri_o ? a1s : -a1c;
        const double c2r = ri_o ? a2c : a2s, c2i = ri_o ? a2s : -a2c;
        A1.a[T] = mfma(c1r, in.v[s_i].x, A1.a[T]);
        A2.a[T] = mfma(c2r, in.v[s_i].x, A2.a[T]);
        A1.a[T] = mfma(c1i, in.v[s_i].y, A1.a[T]);
        A2.a[T] = mfma(c2i, in.v[s_i].y, A2.a[T]);
      }
    }
  }
}

// rmul_acc's four-product chain for a 16-column input tile and an M-column output (the updates with a basis of another
// width, kernels_basis.hip and kernels_basis_slice_axpy.hip): the 16 rows of C that belong to the input tile are staged at
// Ml[j_in * LD + 2 j_out + comp], LD = 2 M + 1 (the padded layout of MatLds<M>).
template <int M>
__device__ __forceinline__ void rect_acc(Acc<M>& A, const Tile<16>& in, const double* Ml, int lane) {
  constexpr int LD = MatLds<M>::LD;
  const int kq = lane >> 4;
  const int ar = lane & 15;
#pragma unroll
  for (int T = 0; T < M / 8; ++T) {
    const int q_o = 4 * T + (ar >> 2);
    const int s_o = q_o % (M / 4);
    const int j_o = 4 * s_o + (ar & 3);
    const double* base = Ml + kq * LD + 2 * j_o;
#pragma unroll
    for (int s_i = 0; s_i < 4; ++s_i) {
      const double a_same = base[s_i * 4 * LD + 0];   // Re C(j_i, j_o)
      const double a_cross = base[s_i * 4 * LD + 1];  // Im C(j_i, j_o)
      if (T < M / 16) {
        A.a[T] = mfma(a_same, in.v[s_i].x, A.a[T]);
        A.a[T] = mfma_nega(a_cross, in.v[s_i].y, A.a[T]);
      } else {
        A.a[T] = mfma(a_cross, in.v[s_i].x, A.a[T]);
        A.a[T] = mfma(a_same, in.v[s_i].y, A.a[T]);
      }
    }
  }
}

// ---- Gram accumulation ---------------------------------------------------------------------------
// Operands in (row k = l>>4, column n = l&15 [+16 jb]) ownership.  Per j-block pair (ja, jb):
//   re(ja,jb) += a_re*b_re + a_im*b_im ;  im(ja,jb) += a_re*b_im - a_im*b_re      (conj(a) * b)
template <int M>
struct GramAcc {
  d4 re[(M / 16) * (M / 16)];
  d4 im[(M / 16) * (M / 16)];
};
template <int M>
__device__ __forceinline__ void gram_zero(GramAcc<M>& G) {
#pragma unroll
  for (int q = 0; q < (M / 16) * (M / 16); ++q) {
    G.re[q] = d4{0.0, 0.0, 0.0, 0.0};
    G.im[q] = d4{0.0, 0.0, 0.0, 0.0};
  }
}
// a[jb], b[jb]: the lane's complex element of column 16*jb + (l&15) for the wave's 4 rows of this step
template <int M>
__device__ __forceinline__ void gram_step(GramAcc<M>& G, const double2* a, const double2* b) {
  constexpr int JB = M / 16;
#pragma unroll
  for (int ja = 0; ja < JB; ++ja)
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
      const int q = ja * JB + jb;
      G.re[q] = mfma(a[ja].x, b[jb].x, G.re[q]);
      G.re[q] = mfma(a[ja].y, b[jb].y, G.re[q]);
      G.im[q] = mfma(a[ja].x, b[jb].y, G.im[q]);
      G.im[q] = mfma_nega(a[ja].y, b[jb].x, G.im[q]);
    }
}

// Self-product G = a^dagger a at M = 16 (the second factor of the factored stencil pair).  With x = Re a,
// y = Im a:  Re G = x^T x + y^T y,  Im G = C - C^T with C = x^T y -- gram_step's fourth product is the transpose of its
// third.  In every form G.im holds C alone and gram_self_block_store antisymmetrises it.
// Three products (-DBCG_SELF_GRAM_3M, A/B builds): G.re exactly as gram_step(G, a, a) fills it, the same two instructions
// in the same order.
// Two products (the default; Gauss's trick as in rmul_acc): G.re holds P = (x + y)^T (x + y) = Re G + C + C^T and the
// store forms Re G = P - (C + C^T).  One v_add_f64 per call for x + y.  Re G is then a difference of sums of comparable
// size, |error| <= about 3 eps sqrt(G_ii G_jj) per entry where the direct sum has eps -- the size of the rounding the other
// operator form and any other order of the site sum carry (measured: DESIGN.md §4, profiles/r08_self_gram_ab.txt).
// -DBCG_SELF_GRAM_4M (A/B builds): the callers keep gram_step(G, a, a) and gram_block_store (kSelfGramProducts == 4).
#if defined(BCG_SELF_GRAM_4M)
constexpr int kSelfGramProducts = 4;
#elif defined(BCG_SELF_GRAM_3M)
constexpr int kSelfGramProducts = 3;
#else
constexpr int kSelfGramProducts = 2;
#endif
__device__ __forceinline__ void gram_self_step(GramAcc<16>& G, const double2* a) {
  if constexpr (kSelfGramProducts == 2) {
    const double s = a[0].x + a[0].y;
    G.re[0] = mfma(s, s, G.re[0]);
  } else {
    G.re[0] = mfma(a[0].x, a[0].x, G.re[0]);
    G.re[0] = mfma(a[0].y, a[0].y, G.re[0]);
  }
  G.im[0] = mfma(a[0].x, a[0].y, G.im[0]);
}

// Sum the per-wave fragments of a block in wave order and write partials[block][j*M + i].
// red: LDS scratch of NW * JB*JB * 2 * 4 * 64 doubles.
// wt: write-through (sc1) stores -- the partials are handed to another workgroup inside this launch (gram_fold)
__device__ __forceinline__ void st_partial(double2* p, double2 v, bool wt) {
  if (wt) st_sc1(p, v);
  else *p = v;
}
template <int M, int NW>
__device__ __forceinline__ void gram_block_store(const GramAcc<M>& G, double* red, double2* __restrict__ partials, int tid,
                                                 bool wt = false) {
  // one 16 x 16 block of the Gram matrix at a time through a buffer of NW * 8 * 64 doubles (16 KB at four waves): at
  // m = 32 a buffer for all four blocks was 64 KB and left phase B a single block per CU
  constexpr int JB = M / 16;
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int q = 0; q < JB * JB; ++q) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red[(wave * 8 + r) * 64 + lane] = G.re[q][r];
      red[(wave * 8 + 4 + r) * 64 + lane] = G.im[q][r];
    }
    __syncthreads();
    // element e = (r, lane): i = 16*ja + (lane>>4) + 4r, j = 16*jb + (lane&15)
    for (int e = tid; e < 4 * 64; e += NW * 64) {
      const int l = e & 63, r = (e >> 6) & 3;
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        sr += red[(w * 8 + r) * 64 + l];
        si += red[(w * 8 + 4 + r) * 64 + l];
      }
      const int i = 16 * (q / JB) + (l >> 4) + 4 * r, j = 16 * (q % JB) + (l & 15);
      st_partial(partials + static_cast<int64_t>(blockIdx.x) * (M * M) + j * M + i, make_double2(sr, si), wt);
    }
  }
}

// gram_block_store for the accumulators of gram_self_step.  The fragments are summed in wave order as above; the thread
// that writes element (i, j) also sums element (j, i) of C (fragment r' = j>>2, lane 16 (j&3) + i of the same buffer, in
// the same wave order) and writes Im = C(i,j) - C(j,i): Im G_ii == 0 and G_ji == conj(G_ij) hold exactly in every block
// partial (Re G(i,j) and Re G(j,i) are the same chain of the same products), and so in every sum of partials taken in a
// fixed order -- the antisymmetrisation is linear, it commutes with gram_fold and reduce_partials.
template <int NW>
__device__ __forceinline__ void gram_self_block_store(const GramAcc<16>& G, double* red, double2* __restrict__ partials, int tid,
                                                      bool wt = false) {
  const int wave = tid >> 6, lane = tid & 63;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[(wave * 8 + r) * 64 + lane] = G.re[0][r];
    red[(wave * 8 + 4 + r) * 64 + lane] = G.im[0][r];
  }
  __syncthreads();
  for (int e = tid; e < 4 * 64; e += NW * 64) {
    const int l = e & 63, r = (e >> 6) & 3;
    const int i = (l >> 4) + 4 * r, j = l & 15;
    const int lt = 16 * (j & 3) + i, rt = j >> 2;  // element (j, i)
    double sr = 0.0, c = 0.0, ct = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      sr += red[(w * 8 + r) * 64 + l];
      c += red[(w * 8 + 4 + r) * 64 + l];
      ct += red[(w * 8 + 4 + rt) * 64 + lt];
    }
    if constexpr (kSelfGramProducts == 2) sr -= c + ct;
    st_partial(partials + static_cast<int64_t>(blockIdx.x) * 256 + j * 16 + i, make_double2(sr, c - ct), wt);
  }
}

// m = 8 on the 16x16 MFMA tile.  With lane = (row pair k = l>>4, row parity s = (l>>3)&1, column c = l&7) holding the
// element (row 2k+s, column c) of both operands, gram_step<16> accumulates C[(s,i)][(s',j)] = sum_k conj(a(2k+s,i)) b(2k+s',j):
// the two diagonal blocks s = s' are Gram contributions (even and odd rows), the off-diagonal ones are discarded.  So
// the whole m = 16 machinery applies unchanged and only this final store differs: G(i,j) = C[i][j] + C[8+i][8+j].
template <int NW>
__device__ __forceinline__ void gram_block_store_fold8(const GramAcc<16>& G, double* red, double2* __restrict__ partials, int tid,
                                                       bool wt = false) {
  constexpr int FR = 8;  // doubles per lane
  const int wave = tid >> 6, lane = tid & 63;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[((wave * FR) + r) * 64 + lane] = G.re[0][r];
    red[((wave * FR) + 4 + r) * 64 + lane] = G.im[0][r];
  }
  __syncthreads();
  // fragment element (r, l): i16 = (l>>4) + 4r, j16 = l&15.  Block (0,0): r < 2, (l&15) < 8; its partner in block (1,1): (r+2, l+8)
  for (int e = tid; e < 4 * 64; e += NW * 64) {
    const int l = e & 63, r = e >> 6;
    if (r >= 2 || (l & 15) >= 8) continue;
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      sr += red[((w * FR) + r) * 64 + l] + red[((w * FR) + r + 2) * 64 + l + 8];
      si += red[((w * FR) + 4 + r) * 64 + l] + red[((w * FR) + 4 + r + 2) * 64 + l + 8];
    }
    const int i = (l >> 4) + 4 * r, j = l & 7;
    st_partial(partials + static_cast<int64_t>(blockIdx.x) * 64 + j * 8 + i, make_double2(sr, si), wt);
  }
}


// ---- Gram partials folded inside the producing kernel ------------------------------------------------------------
// After a block has written partials[blockIdx.x][NV], the LAST block to finish of each of 8 groups (blocks g, g + 8, ...)
// sums its group's partials in block order into partials[gridDim.x + g], and the last of the 8 groups to finish sums those
// in group order into `out`: a fixed order whatever the arrival order (bitwise reproducible), no separate reduction
// launch.  The hand-off between workgroups uses no cache-wide fence (a release would write back every dirty line these
// kernels have just produced -- measured: +80 us on a 0.22 ms phase B): every handed-off byte is stored write-through
// (sc1; the callers pass wt = true to gram_block_store), every storing wave drains its stores, a block barrier, ONE lane
// takes an agent-scope ticket, and the block whose ticket is the last reads the bytes with sc1 loads (the L1 is bypassed,
// the L2 is the point of coherence for write-through data).
// tickets: 9 words, zero before the first launch; the final block leaves them zero again.  All threads of the block call it.
// Sum of n values p[0], p[stride], ... read with sc1 loads, in index order; eight loads in flight at a time (one load and
// its wait at a time made the fold's tail 128 serial L2 round trips).
__device__ __forceinline__ double2 sum_sc1(const double2* p, int64_t stride, int n) {
  double sr = 0.0, si = 0.0;
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    dv2 r0, r1, r2, r3, r4, r5, r6, r7;
    const double2* q = p + static_cast<int64_t>(k) * stride;
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r0) : "v"(q));
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r1) : "v"(q + stride));
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r2) : "v"(q + 2 * stride));
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r3) : "v"(q + 3 * stride));
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r4) : "v"(q + 4 * stride));
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r5) : "v"(q + 5 * stride));
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r6) : "v"(q + 6 * stride));
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(r7) : "v"(q + 7 * stride));
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7) : : "memory");
    sr += r0.x; si += r0.y; sr += r1.x; si += r1.y; sr += r2.x; si += r2.y; sr += r3.x; si += r3.y;
    sr += r4.x; si += r4.y; sr += r5.x; si += r5.y; sr += r6.x; si += r6.y; sr += r7.x; si += r7.y;
  }
  for (; k < n; ++k) {
    dv2 r;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p + static_cast<int64_t>(k) * stride) : "memory");
    sr += r.x;
    si += r.y;
  }
  return make_double2(sr, si);
}
// gram_fold's block-wide flag: a static LDS word, or (ROLE_IN_DYNAMIC: a kernel whose dynamic LDS is exactly half a CU's
// and must stay two blocks per CU -- the stencil factor fused with phase B) a word of the caller's dynamic LDS
template <bool ROLE_IN_DYNAMIC>
__device__ __forceinline__ int& gram_fold_role(int* dynamic_word) {
  if constexpr (ROLE_IN_DYNAMIC) {
    return *dynamic_word;
  } else {
    __shared__ int s_role_static;
    return s_role_static;
  }
}
template <int NV, bool ROLE_IN_DYNAMIC = false>
__device__ __forceinline__ void gram_fold(const GramFold& gf, double2* __restrict__ partials, int tid, int nthreads,
                                          int* dynamic_word = nullptr) {
  if (gf.out == nullptr) return;
  int& s_role = gram_fold_role<ROLE_IN_DYNAMIC>(dynamic_word);
  const int nb = gridDim.x, g = blockIdx.x & 7;
  const int in_group = (nb - g + 7) >> 3;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's write-through partial stores have reached the L2
  __syncthreads();
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(gf.tickets + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_role = t == static_cast<unsigned>(in_group - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_role) return;
  double2* const level2 = partials + static_cast<int64_t>(nb) * NV;
  for (int v = tid; v < NV; v += nthreads)
    st_sc1(level2 + g * NV + v, sum_sc1(partials + static_cast<int64_t>(g) * NV + v, static_cast<int64_t>(8) * NV, in_group));
  const int groups = nb < 8 ? nb : 8;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned t = __hip_atomic_fetch_add(gf.tickets + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_role = t == static_cast<unsigned>(groups - 1) ? 2 : 0;
  }
  __syncthreads();
  if (s_role != 2) return;
  for (int v = tid; v < NV; v += nthreads) gf.out[v] = sum_sc1(level2 + v, NV, groups);
  if (tid < 9) gf.tickets[tid] = 0u;  // ready for the next launch (stream order makes this visible to it)
}

inline int grid_tiles(int64_t ntiles, int per_block, int cap) {
  int64_t g = (ntiles + per_block - 1) / per_block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return static_cast<int>(g);
}

template <typename K>
void allow_lds(K kernel, size_t bytes) {
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
}

}  // namespace
}  // namespace bcg
