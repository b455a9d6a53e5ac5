// Fused multi-aggregation for the kgx engine (gfx950, wave64): one gather of
// every neighbour row feeds all requested reducers of {sum, mean, max, min,
// std}; the result blocks are concatenated along the feature axis.
//
// No reference counterpart as a whole (the reference reduces one aggregator
// per call); each block restates spmm.hip's single-reducer arithmetic, which
// is the reference's (aggregators.py:48-232): an RN add chain from +0 in CSR
// order, mean = sum / max(count_f32, 1e-8), max as scatter_reduce amax with
// isinf -> 0, min as -amax(-m), std two-pass with the N divisor.
//
// Lane layout as in spmm.hip: a group of G lanes (G = pow2 >= F/VEC, <= 64)
// owns one row or one chunk of a split row; lane l holds features
// (t*G + l)*VEC .. +VEC for t < NT.  U neighbour rows are gathered together,
// unconditionally on clamped indices, and folded in edge order into every
// live accumulator; clamped edges enter as the reducer's identity, so no load
// sits under a lane-dependent branch (spmm.hip's header, kgx_vec.h).  std's
// second pass reuses the gathered registers when the row (chunk) fits one
// U-block and re-gathers otherwise (the row was just read: L2-resident).
//
// Scheduled mode: a chunk of a split row writes its raw state -- chunk sum,
// chunk amax, chunk amax of -m, and for std the chunk's M2 about its own mean
// and its length -- and multi_fixup_kernel folds a row's chunks in chunk
// order: sums and extremes as spmm_fixup_kernel, M2 by the pairwise update
//   M2 = M2a + M2b + d^2 * na*nb/(na+nb),  d = mean_b - mean_a.
// No atomics: results are bit-identical from run to run.
#include "kgx_internal.h"
#include "kgx_vec.h"

namespace kgx {
namespace {

struct MultiArgs {
  const int32_t* rowptr;
  const int32_t* rows;
  int64_t n_rows;
  const int4* items;
  int64_t n_items;
  const int4* split;
  int64_t n_split;
  const int32_t* idx;
  const float* table;  // first column of this launch
  int64_t ld_t;
  int F;       // columns handled by this launch (a slice of Ft)
  int f_base;  // first column of this launch
  int64_t Ft;  // all columns: block stride in out, section stride in a partial
  float* out;  // first column of this launch, block 0
  int64_t ld_o;
  float* partials;  // first column of this launch, section 0
  int64_t ld_p;     // floats per slot: n_sections * Ft (+ 4 with std: the chunk length)
  int64_t n_slots;  // slots the caller's buffer holds: stores past it are dropped
  int G;
  int lgG;
  // block of each reducer in out (-1: not requested), by kgx_reduce id
  int ob[5];
  // section of each accumulator in a partial (-1: not kept): sum, amax, amax of -m, M2
  int ps, px, pn, pm;
  int need_max, need_min;
};

constexpr int kFixB = 4;  // split-row partials loaded together by the fix-up

// gathers in flight per group, as spmm_kernel's (measured there)
template <int NT>
struct Gathers {
  static constexpr int U = NT >= 4 ? 2 : (NT == 2 ? 4 : 6);
};

template <int NT, int VEC>
struct Acc {
  float s[NT][VEC], mx[NT][VEC], mn[NT][VEC], ssd[NT][VEC];
};

// U consecutive edges [e, e+U) of a row ending at `end`: index loads, then the
// row gathers, all unconditional (edges past `end` are clamped to end-1).
template <int U, int VEC, int NT>
__device__ __forceinline__ void gather_block(const MultiArgs& a, int32_t e, int32_t end, const int (&fl)[NT],
                                             float (&v)[U][NT][VEC]) {
  const int n = end - e;
  int32_t c[U];
#pragma unroll
  for (int u = 0; u < U; ++u) c[u] = a.idx[u < n ? e + u : end - 1];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < NT; ++t) vload<VEC>(v[u][t], a.table + row_off(c[u], a.ld_t) + fl[t]);
}

// First pass: one gathered value feeds the sum and both amax chains, in edge order.
template <int U, int VEC, int NT>
__device__ __forceinline__ void fold_first(const MultiArgs& a, const float (&v)[U][NT][VEC], int n,
                                           Acc<NT, VEC>& acc) {
  const float ninf = -__builtin_inff();
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc.s[t][k] = __fadd_rn(acc.s[t][k], u < n ? v[u][t][k] : 0.0f);
  if (a.need_max) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.mx[t][k] = amax_update(acc.mx[t][k], u < n ? v[u][t][k] : ninf);
  }
  if (a.need_min) {  // min = -segment_max(-m)
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc.mn[t][k] = amax_update(acc.mn[t][k], u < n ? -v[u][t][k] : ninf);
  }
}

// std's second pass: ssd += (v - mean)^2 in edge order (spmm_std_kernel).
template <int U, int VEC, int NT>
__device__ __forceinline__ void fold_second(const float (&v)[U][NT][VEC], int n, const float (&mean)[NT][VEC],
                                            Acc<NT, VEC>& acc) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float d = __fsub_rn(v[u][t][k], mean[t][k]);
        acc.ssd[t][k] = __fadd_rn(acc.ssd[t][k], u < n ? __fmul_rn(d, d) : 0.0f);
      }
}

template <int VEC, int NT, bool STD>
__global__ __launch_bounds__(kBlock) void multi_kernel(MultiArgs a) {
  constexpr int U = Gathers<NT>::U;
  constexpr int TU = U / 2;  // tail in half-width blocks, as spmm_kernel
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const int64_t ngroups = (int64_t(gridDim.x) * kBlock) >> a.lgG;
  const int64_t n_work = a.items ? a.n_items : a.n_rows;

  int fo[NT], fl[NT];
  bool fv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    fo[t] = (t * G + lane) * VEC;
    fv[t] = fo[t] < a.F;
    fl[t] = fv[t] ? fo[t] : a.F - VEC;  // load offset, always in range
  }

  for (int64_t it = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> a.lgG; it < n_work; it += ngroups) {
    int32_t row, beg, end, slot;
    if (a.items) {
      const int4 v = a.items[it];
      row = v.x;
      beg = v.y;
      end = v.z;
      slot = v.w;
    } else {
      row = a.rows[it];
      beg = a.rowptr[row];
      end = a.rowptr[row + 1];
      slot = -1;
    }
    const int32_t n = end - beg;  // the row's degree, or the chunk's length
    const float cnt = ref_count_f32(n);
    const float safe = fmaxf(cnt, 1e-8f);

    Acc<NT, VEC> acc;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        acc.s[t][k] = 0.0f;
        acc.mx[t][k] = acc.mn[t][k] = -__builtin_inff();
        acc.ssd[t][k] = 0.0f;
      }
    float mean[NT][VEC];

    if (STD && n <= U) {
      // the whole row (chunk) is one U-block: both passes from the same registers
      if (n > 0) {
        float v[U][NT][VEC];
        gather_block<U, VEC, NT>(a, beg, end, fl, v);
        fold_first<U, VEC, NT>(a, v, n, acc);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int k = 0; k < VEC; ++k) mean[t][k] = __fdiv_rn(acc.s[t][k], safe);
        fold_second<U, VEC, NT>(v, n, mean, acc);
      }
    } else {
      int32_t e = beg;
      for (; e + U <= end; e += U) {
        float v[U][NT][VEC];
        gather_block<U, VEC, NT>(a, e, end, fl, v);
        fold_first<U, VEC, NT>(a, v, U, acc);
      }
      for (; e < end; e += TU) {
        float v[TU][NT][VEC];
        gather_block<TU, VEC, NT>(a, e, end, fl, v);
        fold_first<TU, VEC, NT>(a, v, end - e, acc);
      }
      if constexpr (STD) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int k = 0; k < VEC; ++k) mean[t][k] = __fdiv_rn(acc.s[t][k], safe);
        e = beg;
        for (; e + U <= end; e += U) {
          float v[U][NT][VEC];
          gather_block<U, VEC, NT>(a, e, end, fl, v);
          fold_second<U, VEC, NT>(v, U, mean, acc);
        }
        for (; e < end; e += TU) {
          float v[TU][NT][VEC];
          gather_block<TU, VEC, NT>(a, e, end, fl, v);
          fold_second<TU, VEC, NT>(v, end - e, mean, acc);
        }
      }
    }

    if (slot >= 0) {  // chunk of a split row: raw state, finished by the fix-up
      if (slot >= a.n_slots) continue;
      float* p = a.partials + int64_t(slot) * a.ld_p;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (!fv[t]) continue;
        if (a.ps >= 0) vstore<VEC>(p + a.ps * a.Ft + fo[t], acc.s[t]);
        if (a.px >= 0) vstore<VEC>(p + a.px * a.Ft + fo[t], acc.mx[t]);
        if (a.pn >= 0) vstore<VEC>(p + a.pn * a.Ft + fo[t], acc.mn[t]);
        if constexpr (STD) vstore<VEC>(p + a.pm * a.Ft + fo[t], acc.ssd[t]);
      }
      if constexpr (STD) {  // the chunk's length, after the sections (first column slice only)
        if (lane == 0 && a.f_base == 0) p[a.ld_p - 4 - a.f_base] = float(n);
      }
      continue;
    }

    float* o = a.out + int64_t(row) * a.ld_o;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (!fv[t]) continue;
      float r[VEC];
      if (a.ob[KGX_SUM] >= 0) vstore<VEC>(o + a.ob[KGX_SUM] * a.Ft + fo[t], acc.s[t]);
      if (a.ob[KGX_MEAN] >= 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) r[k] = __fdiv_rn(acc.s[t][k], safe);
        vstore<VEC>(o + a.ob[KGX_MEAN] * a.Ft + fo[t], r);
      }
      if (a.ob[KGX_MAX] >= 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) r[k] = is_inf(acc.mx[t][k]) ? 0.0f : acc.mx[t][k];
        vstore<VEC>(o + a.ob[KGX_MAX] * a.Ft + fo[t], r);
      }
      if (a.ob[KGX_MIN] >= 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float m = -acc.mn[t][k];
          r[k] = is_inf(m) ? 0.0f : m;
        }
        vstore<VEC>(o + a.ob[KGX_MIN] * a.Ft + fo[t], r);
      }
      if constexpr (STD) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float var = __fdiv_rn(acc.ssd[t][k], safe);
          const float sd = sqrt_rn(fmaxf(var, 0.0f) /* maximum(variance, 0) */);
          r[k] = cnt <= 1.0f ? 0.0f : (var != var ? var : sd);
        }
        vstore<VEC>(o + a.ob[KGX_STD] * a.Ft + fo[t], r);
      }
    }
  }
}

// Fold the chunk states of split rows in chunk order, then finish every block.
template <int VEC, bool STD>
__global__ __launch_bounds__(kBlock) void multi_fixup_kernel(MultiArgs a) {
  const int G = a.G;
  const int lane = threadIdx.x & (G - 1);
  const int64_t ngroups = (int64_t(gridDim.x) * kBlock) >> a.lgG;
  const float ninf = -__builtin_inff();
  for (int64_t it = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> a.lgG; it < a.n_split; it += ngroups) {
    const int4 s = a.split[it];
    const int32_t row = s.x, slot0 = s.y, nc = s.z, deg = s.w;
    if (nc <= 0 || slot0 < 0 || int64_t(slot0) + nc > a.n_slots) continue;
    const float cnt = ref_count_f32(deg);
    const float safe = fmaxf(cnt, 1e-8f);
    const float* p0 = a.partials + int64_t(slot0) * a.ld_p;
    float* o = a.out + int64_t(row) * a.ld_o;
    for (int f = lane * VEC; f < a.F; f += G * VEC) {
      float sum[VEC], mx[VEC], mn[VEC], m2[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        sum[k] = m2[k] = 0.0f;
        mx[k] = mn[k] = ninf;
      }
      float na = 0.0f;  // edges folded so far (chunk lengths are < 2^24: exact)
      for (int32_t c0 = 0; c0 < nc; c0 += kFixB) {
        float qs[kFixB][VEC], qx[kFixB][VEC], qn[kFixB][VEC], qm[kFixB][VEC], nb[kFixB];
#pragma unroll
        for (int u = 0; u < kFixB; ++u) {  // clamped, unconditional (the flags are wave-uniform)
          const float* p = p0 + int64_t(c0 + u < nc ? c0 + u : nc - 1) * a.ld_p;
          if (a.ps >= 0) vload<VEC>(qs[u], p + a.ps * a.Ft + f);
          if (a.px >= 0) vload<VEC>(qx[u], p + a.px * a.Ft + f);
          if (a.pn >= 0) vload<VEC>(qn[u], p + a.pn * a.Ft + f);
          if constexpr (STD) {
            vload<VEC>(qm[u], p + a.pm * a.Ft + f);
            nb[u] = p[a.ld_p - 4 - a.f_base];
          }
        }
#pragma unroll
        for (int u = 0; u < kFixB; ++u) {
          const bool live = c0 + u < nc;
          if constexpr (STD) {
            // M2 = M2a + M2b + d^2 na nb / (na + nb), d = mean_b - mean_a; the first chunk's M2 as it is
            const float nab = na + nb[u];
            const float wgt = __fdiv_rn(__fmul_rn(na, nb[u]), nab);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              const float d = __fsub_rn(__fdiv_rn(qs[u][k], nb[u]), __fdiv_rn(sum[k], fmaxf(na, 1.0f)));
              const float merged = __fadd_rn(__fadd_rn(m2[k], qm[u][k]), __fmul_rn(__fmul_rn(d, d), wgt));
              m2[k] = live ? (na > 0.0f ? merged : qm[u][k]) : m2[k];
            }
            na = live ? nab : na;
          }
          if (a.ps >= 0) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) sum[k] = live ? __fadd_rn(sum[k], qs[u][k]) : sum[k];
          }
          if (a.px >= 0) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) mx[k] = live ? amax_update(mx[k], qx[u][k]) : mx[k];
          }
          if (a.pn >= 0) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) mn[k] = live ? amax_update(mn[k], qn[u][k]) : mn[k];
          }
        }
      }
      float r[VEC];
      if (a.ob[KGX_SUM] >= 0) vstore<VEC>(o + a.ob[KGX_SUM] * a.Ft + f, sum);
      if (a.ob[KGX_MEAN] >= 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) r[k] = __fdiv_rn(sum[k], safe);
        vstore<VEC>(o + a.ob[KGX_MEAN] * a.Ft + f, r);
      }
      if (a.ob[KGX_MAX] >= 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) r[k] = is_inf(mx[k]) ? 0.0f : mx[k];
        vstore<VEC>(o + a.ob[KGX_MAX] * a.Ft + f, r);
      }
      if (a.ob[KGX_MIN] >= 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float m = -mn[k];
          r[k] = is_inf(m) ? 0.0f : m;
        }
        vstore<VEC>(o + a.ob[KGX_MIN] * a.Ft + f, r);
      }
      if constexpr (STD) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float var = __fdiv_rn(m2[k], safe);
          const float sd = sqrt_rn(fmaxf(var, 0.0f));
          r[k] = cnt <= 1.0f ? 0.0f : (var != var ? var : sd);
        }
        vstore<VEC>(o + a.ob[KGX_STD] * a.Ft + f, r);
      }
    }
  }
}

template <int VEC, int NT, bool STD>
int launch(const MultiArgs& a, hipStream_t s) {
  const int64_t n_work = a.items ? a.n_items : a.n_rows;
  if (n_work > 0) {
    auto k = multi_kernel<VEC, NT, STD>;
    hipLaunchKernelGGL(k, dim3(resident_grid(k, n_work, a.G)), dim3(kBlock), 0, s, a);
    KGX_CHECK_LAUNCH();
  }
  if (a.items && a.n_split > 0) {
    auto k = multi_fixup_kernel<VEC, STD>;
    hipLaunchKernelGGL(k, dim3(resident_grid(k, a.n_split, a.G)), dim3(kBlock), 0, s, a);
    KGX_CHECK_LAUNCH();
  }
  return KGX_OK;
}

template <int VEC>
int dispatch(int nt, bool with_std, const MultiArgs& a, hipStream_t s) {
  if (with_std) {
    if (nt == 1) return launch<VEC, 1, true>(a, s);
    if (nt == 2) return launch<VEC, 2, true>(a, s);
    return launch<VEC, 4, true>(a, s);
  }
  if (nt == 1) return launch<VEC, 1, false>(a, s);
  if (nt == 2) return launch<VEC, 2, false>(a, s);
  return launch<VEC, 4, false>(a, s);
}

bool aligned(const void* p, int bytes) { return p == nullptr || reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// Which accumulators the reducer list keeps, validated: false on a bad list.
struct Plan {
  int ob[5] = {-1, -1, -1, -1, -1};
  int ps = -1, px = -1, pn = -1, pm = -1;
  int sections = 0;
  bool with_std = false;
};

bool make_plan(int n_red, const int* reduces, Plan& p) {
  if (!reduces || n_red < 1 || n_red > 5) return false;
  for (int k = 0; k < n_red; ++k) {
    const int r = reduces[k];
    if (r < KGX_SUM || r > KGX_STD || p.ob[r] >= 0) return false;
    p.ob[r] = k;
  }
  p.with_std = p.ob[KGX_STD] >= 0;
  if (p.ob[KGX_SUM] >= 0 || p.ob[KGX_MEAN] >= 0 || p.with_std) p.ps = p.sections++;
  if (p.ob[KGX_MAX] >= 0) p.px = p.sections++;
  if (p.ob[KGX_MIN] >= 0) p.pn = p.sections++;
  if (p.with_std) p.pm = p.sections++;
  return true;
}

int64_t slot_floats(const Plan& p, int64_t F) { return p.sections * F + (p.with_std ? 4 : 0); }

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" int kgx_multi_aggr_partials_floats(int n_red, const int* reduces, int64_t n_slots, int64_t F,
                                              int64_t* floats) {
  Plan p;
  KGX_REQUIRE(make_plan(n_red, reduces, p), KGX_ERR_ARG,
              "kgx_multi_aggr_partials_floats: 1..5 distinct kgx_reduce ids expected");
  KGX_REQUIRE(n_slots >= 0 && F >= 0 && floats, KGX_ERR_ARG, "kgx_multi_aggr_partials_floats: bad arguments");
  *floats = n_slots * slot_floats(p, F);
  return KGX_OK;
}

extern "C" int kgx_multi_aggr(int n_red, const int* reduces, const int32_t* rowptr, const int32_t* rows,
                              int64_t n_rows, const int32_t* items, int64_t n_items, const int32_t* split,
                              int64_t n_split, const int32_t* idx, const float* table, int64_t ld_table, int64_t F,
                              float* out, int64_t ld_out, float* partials, int64_t partials_floats,
                              kgx_stream_t stream_) {
  Plan p;
  KGX_REQUIRE(reduces, KGX_ERR_ARG, "kgx_multi_aggr: null reduces");
  KGX_REQUIRE(n_red >= 1 && n_red <= 5, KGX_ERR_ARG, "kgx_multi_aggr: n_red %d outside 1..5", n_red);
  KGX_REQUIRE(make_plan(n_red, reduces, p), KGX_ERR_ARG, "kgx_multi_aggr: unknown or repeated reduce id");
  KGX_REQUIRE(F >= 0 && n_rows >= 0 && n_items >= 0 && n_split >= 0 && partials_floats >= 0 && ld_table >= 0 &&
                  ld_out >= 0,
              KGX_ERR_ARG, "kgx_multi_aggr: negative size");
  KGX_REQUIRE(rowptr && rows && idx && table && out, KGX_ERR_ARG, "kgx_multi_aggr: null CSR / table / out pointer");
  KGX_REQUIRE(ld_out >= int64_t(n_red) * F, KGX_ERR_ARG, "kgx_multi_aggr: ld_out %lld < n_red * F = %lld",
              (long long)ld_out, (long long)(int64_t(n_red) * F));
  KGX_REQUIRE(ld_table >= F && ld_table < (int64_t(1) << 31), KGX_ERR_ARG,
              "kgx_multi_aggr: table leading dimension %lld outside [F, 2^31)", (long long)ld_table);
  const int64_t ld_p = slot_floats(p, F);
  const bool fix = items != nullptr && n_split > 0;
  KGX_REQUIRE(!fix || (split && partials), KGX_ERR_ARG, "kgx_multi_aggr: split rows need split list and partials");
  // every split row has at least one chunk: fewer slots than split rows cannot be right
  KGX_REQUIRE(!fix || (ld_p > 0 && partials_floats / ld_p >= n_split), KGX_ERR_ARG,
              "kgx_multi_aggr: partials_floats %lld too small (see kgx_multi_aggr_partials_floats)",
              (long long)partials_floats);
  if (F == 0 || n_rows == 0) return KGX_OK;
  hipStream_t stream = as_stream(stream_);

  MultiArgs a{};
  a.rowptr = rowptr;
  a.rows = rows;
  a.n_rows = n_rows;
  a.items = reinterpret_cast<const int4*>(items);
  a.n_items = items ? n_items : 0;
  a.split = reinterpret_cast<const int4*>(split);
  a.n_split = fix ? n_split : 0;
  a.idx = idx;
  a.ld_t = ld_table;
  a.Ft = F;
  a.ld_o = ld_out;
  a.ld_p = ld_p;
  a.n_slots = fix ? partials_floats / ld_p : 0;
  for (int r = 0; r < 5; ++r) a.ob[r] = p.ob[r];
  a.ps = p.ps;
  a.px = p.px;
  a.pn = p.pn;
  a.pm = p.pm;
  a.need_max = p.ob[KGX_MAX] >= 0;
  a.need_min = p.ob[KGX_MIN] >= 0;

  // widest vector the shapes and pointers allow
  auto ok = [&](int v) {
    return F % v == 0 && ld_table % v == 0 && ld_out % v == 0 && aligned(table, 4 * v) && aligned(out, 4 * v) &&
           aligned(partials, 4 * v);
  };
  const int VEC = ok(4) ? 4 : (ok(2) ? 2 : 1);
  const int64_t fvec = F / VEC;
  const int G = int(fvec >= 64 ? 64 : next_pow2(int(fvec)));
  // column slices of at most 4*64*VEC features per launch
  const int64_t slice = int64_t(4) * 64 * VEC;
  for (int64_t c0 = 0; c0 < F; c0 += slice) {
    const int64_t cw = (F - c0) < slice ? (F - c0) : slice;
    const int64_t cv = cw / VEC;
    const int nt = cv <= 64 ? 1 : (cv <= 128 ? 2 : 4);
    MultiArgs s = a;
    s.F = int(cw);
    s.f_base = int(c0);
    s.G = G;
    s.lgG = log2i(G);
    s.table = table + c0;
    s.out = out + c0;
    s.partials = partials ? partials + c0 : nullptr;
    int rc;
    if (VEC == 4) rc = dispatch<4>(nt, p.with_std, s, stream);
    else if (VEC == 2) rc = dispatch<2>(nt, p.with_std, s, stream);
    else rc = dispatch<1>(nt, p.with_std, s, stream);
    if (rc != KGX_OK) return rc;
  }
  return KGX_OK;
}
