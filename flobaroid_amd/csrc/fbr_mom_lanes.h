// fbr_mom_lanes.h -- the wave-wide sum of the rhs moments of a column group (producer fbr_kinimg_kernel, fbr_gram64.h), written once for
// the device and for the CPU emulation (tests/emul/gram64_mom_lanes.cpp).  No HIP in this file: the exchanges come from a functor.
//
// fbr_mom_lanes_sum<NQ>(v, live, x): every lane brings its NQ values v[0 .. NQ) (one per column of the group) and its flag `live`; the
// result r holds, in EVERY lane of the class of column c (fbr_mom_lanes_class), the sum of v[c] over the live lanes of the wave.
//
// Dead lanes (behind the last sample of a partly filled block).  The producer runs ALL 64 lanes -- a dead lane walks the tree on the
// block's last sample, so its registers are defined -- and this function replaces a dead lane's values by +0.0 with a SELECT (never a
// product: a NaN or an infinity in a dead lane must not get through) before the first exchange.  The other form, keeping the dead
// lanes switched off, was not taken: what an exchange reads from a disabled lane differs from instruction to instruction (a DPP move
// can be told to read zero, a row swap moves registers of disabled lanes or does not), and a rule per instruction is easy to get
// wrong; with all lanes running, every exchange reads a defined value whatever it is built from.
//
// Order of the additions (fixed; T + T is IEEE addition, which commutes, so both partners of an exchange get the same bits).  With
// x_c[i] = live[i] ? v[c] of lane i : 0:
//   halves   a[i] = x[i] + x[i + 32]                i < 32
//   rows     b[i] = a[i] + a[i + 16]                i < 16
//   in a row c8[i] = b[i] + b[i ^ 8],  c7[i] = c8[i] + c8[i ^ 7],  c2[i] = c7[i] + c7[i ^ 2],  sum = c2[i] + c2[i ^ 1]   (any i < 16: all equal)
// The columns are split between the partners of the first exchanges, so that a group costs about NQ / 2 + NQ / 4 + 4 additions and not 6
// per column: of n values, h = (n + 1) / 2 survive an exchange; the lanes with the exchange's bit clear keep values [0, h), the lanes with
// the bit set keep values [h, n) as their values [0, n - h) and zeros behind them.  Halves (bit 32) split first, rows (bit 16) second;
// two values that are left after the rows (NQ > 4) are summed in the row both, and bit 8 of the lane says which one the lane returns.
//
// The functor x:
//   x.swap32(a, b) / x.swap16(a, b)   the lanes with the bit set hand their a to their partner (lane ^ bit) and take its b:
//                                     a'[i] = bit(i) ? b[i ^ bit] : a[i],   b'[i] = bit(i) ? b[i] : a[i ^ bit]
//   x.get8 / get7 / get2 / get1 (a)   the value of a in lane i ^ 8 / 7 / 2 / 1
//   x.live0(live, a)                  live ? a : +0.0
//   x.bit8(a, b)                      (lane & 8) ? b : a
//   x.zero()                          +0.0 in every lane
#pragma once
#include "fbr_math.h"

// the column whose sum lane `lane` holds after fbr_mom_lanes_sum<NQ>, or -1 (the lane holds the sum of zeros)
FBR_HD int fbr_mom_lanes_class(int nq, int lane)
{
    const int h32 = (nq + 1) / 2, h16 = (h32 + 1) / 2;  // values left after the halves / the rows (h16: 1, or 2 for nq > 4)
    const int i8 = h16 > 1 ? (lane >> 3) & 1 : 0;
    const int i16 = h32 > 1 ? i8 + h16 * ((lane >> 4) & 1) : 0;  // (a single value is not split: both partners keep its sum)
    if (i16 >= h32) return -1;
    const int c = nq > 1 ? i16 + h32 * ((lane >> 5) & 1) : 0;
    return c < nq ? c : -1;
}

// The lane that adds parameter pidx (0 .. 9) of a link to its running sum for rhs column r (0, 1).  The producer sums parameters 0 .. 3 as a
// group of four and 4 .. 9 as a group of six (a smaller group sits at its place in these with zeros around it), so the lane is in the class
// of column pidx of fbr_mom_lanes_sum<4> or of column pidx - 4 of fbr_mom_lanes_sum<6>: 0 16 32 48 | 1 9 17 33 41 49 for r = 0 and six lanes
// further on for r = 1 (same classes) -- twenty different lanes, so that ONE register pair collects a link's sums and ONE atomic adds them.
// fbr_gram64_mom_fric_lane: the (up to four) friction columns of the link's joint, 2 .. 5 and 10 .. 13 (one value per sum: any lane has it).
FBR_HD int fbr_gram64_mom_lane(int pidx, int r = 0)
{
    if (pidx < 4) return 16 * pidx + 6 * r;
    const int q = pidx - 4;
    return 32 * (q / 3) + 8 * (q % 3) + 1 + 6 * r;
}
FBR_HD int fbr_gram64_mom_fric_lane(int pf, int r = 0) { return 2 + pf + 8 * r; }

template <int NQ, class T, class L, class X>
FBR_HD T fbr_mom_lanes_sum(const T *v, const L &live, X &x)
{
    static_assert(NQ >= 1 && NQ <= 8, "two split exchanges and bit 8 tell at most eight columns apart");
    constexpr int H32 = (NQ + 1) / 2, H16 = (H32 + 1) / 2;
    T a[H32], b[H16];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < H32; i++) {
        a[i] = x.live0(live, v[i]);
        T up = i + H32 < NQ ? x.live0(live, v[i + H32]) : (NQ == 1 ? a[i] : x.zero());  // (one column: both halves keep it)
        x.swap32(a[i], up);
        a[i] = a[i] + up;
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < H16; i++) {
        b[i] = a[i];
        T up = i + H16 < H32 ? a[i + H16] : (H32 == 1 ? a[i] : x.zero());
        x.swap16(b[i], up);
        b[i] = b[i] + up;
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < H16; i++) {
        b[i] = b[i] + x.get8(b[i]);
        b[i] = b[i] + x.get7(b[i]);
        b[i] = b[i] + x.get2(b[i]);
        b[i] = b[i] + x.get1(b[i]);
    }
    if constexpr (H16 > 1)
        return x.bit8(b[0], b[1]);
    else
        return b[0];
}
