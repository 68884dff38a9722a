// The device pieces that the message kernels share (lpa_agg.hip, lpa_pregel.hip): the message
// interpreter am_eval, a lane's partial AmRow with its merge and its xor-shuffle tree, the
// order-free min and max, the list views and the offsets of the message lists.  lpa_agg.hip's
// header describes the interpreter, the null rules and the shape of a row's reduction.  Everything
// here has internal linkage: each of the two files gets its own copy.  Contraction into fused
// multiply-adds is off from here on: a message is the double that numpy computes op by op.
#pragma once

#include <math.h>

#include "lpa_device.h"
#include "lpa_algo.h"

#pragma clang fp contract(off)

namespace lpa {

namespace {

constexpr int kAmLdsSlots = LPA_AM_MAX_STACK - 1;   // the top of the stack is a register
constexpr int kAmGrid = 2048;                        // blocks of the short and the wave launch at most

struct AmIn {
  const lpa_am_program* prog;   // device [2]: [0] to_src, [1] to_dst
  const double* vcols;          // [n_vcols][V]
  const double* ecols;          // [n_ecols][m]
  int64_t V, m;
};

struct AmLists {   // a direction that is not in use: null pointers
  const int64_t *io, *oo;
  const int32_t *icol, *ocol;
  const int64_t *ieid, *oeid;
};

struct AmRow {   // a lane's (then a row's) partial
  u32 c_dst, c_src;   // delivered messages by direction
  double sum, mn, mx;
};

__device__ __forceinline__ AmRow am_empty() { return AmRow{0u, 0u, 0.0, INFINITY, -INFINITY}; }

// -0.0 below +0.0: the result does not depend on the order of the operands
__device__ __forceinline__ double am_min(double a, double b) {
  return a < b || (a == b && __builtin_signbit(a)) ? a : b;
}
__device__ __forceinline__ double am_max(double a, double b) {
  return a > b || (a == b && !__builtin_signbit(a)) ? a : b;
}

__device__ __forceinline__ void am_merge(AmRow& a, const AmRow& b) {
  a.c_dst += b.c_dst;
  a.c_src += b.c_src;
  a.sum += b.sum;
  a.mn = am_min(a.mn, b.mn);
  a.mx = am_max(a.mx, b.mx);
}

// the partials of the `width` neighbouring lanes combined in every one of them
template <int kWidth>
__device__ __forceinline__ void am_tree(AmRow& a) {
#pragma unroll
  for (int off = kWidth / 2; off > 0; off >>= 1) {
    AmRow b;
    b.c_dst = (u32)__shfl_xor((int)a.c_dst, off, 64);
    b.c_src = (u32)__shfl_xor((int)a.c_src, off, 64);
    b.sum = __shfl_xor(a.sum, off, 64);
    b.mn = __shfl_xor(a.mn, off, 64);
    b.mx = __shfl_xor(a.mx, off, 64);
    am_merge(a, b);
  }
}

// One message: the program P over the edge row e from s to d.  True when it is not null, *out
// its value.  stk: this thread's column of the LDS stack, kNT doubles from slot to slot.
template <int kNT>
__device__ __forceinline__ bool am_eval(const lpa_am_program* __restrict__ P, const AmIn& in, int64_t s, int64_t d,
                                        int64_t e, double* stk, double* out) {
  double t = 0.0;   // the top of the stack; the value at depth i < sp - 1 is stk[i * kNT]
  u32 vb = 0;       // bit i: the value at depth i is not null
  int sp = 0;
  const int n = P->n_ops;
  for (int pc = 0; pc < n; ++pc) {
    const u32 w = P->ops[pc];
    const u32 op = w & 0xFFFFu, arg = w >> 16;
    if (op <= LPA_AM_EDGE) {   // the pushes
      if (sp > 0) stk[(sp - 1) * kNT] = t;
      switch (op) {
        case LPA_AM_CONST: t = P->consts[arg]; break;
        case LPA_AM_SRC: t = in.vcols[(int64_t)arg * in.V + s]; break;
        case LPA_AM_DST: t = in.vcols[(int64_t)arg * in.V + d]; break;
        default: t = in.ecols[(int64_t)arg * in.m + e]; break;
      }
      vb |= 1u << sp;
      ++sp;
    } else if (op == LPA_AM_NEG) {
      t = -t;
    } else if (op == LPA_AM_ABS) {
      t = __builtin_fabs(t);
    } else if (op == LPA_AM_NOT) {
      t = t != 0.0 ? 0.0 : 1.0;
    } else if (op == LPA_AM_WHEN_ELSE) {   // condition, value, otherwise
      const double c = stk[(sp - 3) * kNT], x = stk[(sp - 2) * kNT];
      const bool take = ((vb >> (sp - 3)) & 1u) && c != 0.0;
      const bool ok = take ? (vb >> (sp - 2)) & 1u : (vb >> (sp - 1)) & 1u;
      t = take ? x : t;
      sp -= 2;
      vb = (vb & ((1u << (sp - 1)) - 1u)) | ((ok ? 1u : 0u) << (sp - 1));
    } else {   // the binary ops
      const double a = stk[(sp - 2) * kNT], b = t;
      bool ok = ((vb >> (sp - 2)) & (vb >> (sp - 1)) & 1u) != 0;
      switch (op) {
        case LPA_AM_ADD: t = a + b; break;
        case LPA_AM_SUB: t = a - b; break;
        case LPA_AM_MUL: t = a * b; break;
        case LPA_AM_DIV: t = a / b; ok = ok && b != 0.0; break;
        case LPA_AM_EQ: t = a == b ? 1.0 : 0.0; break;
        case LPA_AM_NE: t = a != b ? 1.0 : 0.0; break;
        case LPA_AM_LT: t = a < b ? 1.0 : 0.0; break;
        case LPA_AM_LE: t = a <= b ? 1.0 : 0.0; break;
        case LPA_AM_GT: t = a > b ? 1.0 : 0.0; break;
        case LPA_AM_GE: t = a >= b ? 1.0 : 0.0; break;
        case LPA_AM_AND: t = a != 0.0 && b != 0.0 ? 1.0 : 0.0; break;
        case LPA_AM_OR: t = a != 0.0 || b != 0.0 ? 1.0 : 0.0; break;
        default:   // LPA_AM_WHEN: condition, value
          ok = ((vb >> (sp - 2)) & 1u) && a != 0.0 && ((vb >> (sp - 1)) & 1u);
          break;
      }
      sp -= 1;
      vb = (vb & ((1u << (sp - 1)) - 1u)) | ((ok ? 1u : 0u) << (sp - 1));
    }
  }
  *out = t;
  return (vb & 1u) != 0;
}

__device__ __forceinline__ void am_take(AmRow& a, bool ok, double x, u32& c) {
  if (ok) {
    ++c;
    a.sum += x;
    a.mn = am_min(a.mn, x);
    a.mx = am_max(a.mx, x);
  }
}

__device__ __forceinline__ int64_t am_len(const AmLists& l, int64_t v) {
  return (l.io ? l.io[v + 1] - l.io[v] : 0) + (l.oo ? l.oo[v + 1] - l.oo[v] : 0);
}

// cnt[0] += messages delivered to destinations, [1] to sources, [2] receivers: a thread's totals,
// three atomics per wave at the kernel's end
__device__ __forceinline__ void am_counts(ull* __restrict__ cnt, ull n_dst, ull n_src, ull n_recv) {
  for (int off = 32; off > 0; off >>= 1) {
    n_dst += __shfl_xor(n_dst, off, 64);
    n_src += __shfl_xor(n_src, off, 64);
    n_recv += __shfl_xor(n_recv, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_dst) atomicAdd(&cnt[0], n_dst);
    if (n_src) atomicAdd(&cnt[1], n_src);
    if (n_recv) atomicAdd(&cnt[2], n_recv);
  }
}

// off[v], v in [0, V]: the first entry of v's message list; cnt[3] = the longest list
__global__ __launch_bounds__(256) void k_am_offsets(AmLists l, int64_t V, int64_t* __restrict__ off,
                                                    ull* __restrict__ cnt) {
  ull lmax = 0;
  GRID_STRIDE(v, V + 1) {
    off[v] = (l.io ? l.io[v] : 0) + (l.oo ? l.oo[v] : 0);
    if (v < V) {
      const ull L = (ull)am_len(l, v);
      lmax = L > lmax ? L : lmax;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const ull x = __shfl_xor(lmax, o, 64);
    lmax = x > lmax ? x : lmax;
  }
  if ((threadIdx.x & 63) == 0 && lmax) atomicMax(&cnt[3], lmax);
}

}  // namespace

}  // namespace lpa
