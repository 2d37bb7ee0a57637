// Argument checks shared by flock_vdn_act and flock_maddpg_act, plain C++. `op`: the entry's name, the messages' prefix
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "learn_internal.h"

namespace flock_act_host {

inline int fail_op(int code, const char* op, const char* msg) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", op, msg);
    return flock_learn_internal::fail(code, buf);
}

// [lo, hi) bytes covered by rows b < B, agents a < A of `width` floats at base + b*sr + a*sa
inline void extent(const float* base, int A, int B, int64_t sr, int64_t sa, int width, uintptr_t& lo, uintptr_t& hi) {
    const int64_t dr = (int64_t)(B - 1) * sr, da = (int64_t)(A - 1) * sa;
    const int64_t mn = (dr < 0 ? dr : 0) + (da < 0 ? da : 0), mx = (dr > 0 ? dr : 0) + (da > 0 ? da : 0);
    lo = (uintptr_t)(base + mn);
    hi = (uintptr_t)(base + mx + width);
}

// h_in / h_out [B, A, width] (strides in floats): rows 16-byte aligned (moved with 16-B accesses), buffers disjoint
inline int check_hidden_pair(const char* op, int A, int B, int width, const float* h_in, int64_t h_in_sb,
                             int64_t h_in_sa, const float* h_out, int64_t h_out_sb, int64_t h_out_sa) {
    if (((uintptr_t)h_in | (uintptr_t)h_out) & 15u || ((h_in_sb | h_in_sa | h_out_sb | h_out_sa) & 3))
        return fail_op(-5, op, "hidden rows must be 16-byte aligned");
    uintptr_t ilo, ihi, olo, ohi;
    extent(h_in, A, B, h_in_sb, h_in_sa, width, ilo, ihi);
    extent(h_out, A, B, h_out_sb, h_out_sa, width, olo, ohi);
    if (ilo < ohi && olo < ihi) return fail_op(-5, op, "h_out overlaps h_in (keep two buffers and swap them)");
    return 0;
}

// S = blocks per agent (the grid is A * S): row_split, or at 0 about `target` work items in all, at most one a tile
inline int row_split_of(const char* op, int A, int B, int rows, int row_split, int target, int& S) {
    const int tiles = (int)(((int64_t)B + rows - 1) / rows);
    if (row_split < 0 || (int64_t)A * (row_split ? row_split : tiles) > INT32_MAX)
        return fail_op(-5, op, "row_split must be >= 0 and A * row_split fit the grid");
    S = row_split;
    if (S == 0) {
        S = (int)(((int64_t)target + A - 1) / A);
        if (S > tiles) S = tiles;
    }
    return 0;
}

}  // namespace flock_act_host
