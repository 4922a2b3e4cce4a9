// gram64_mom_lanes.cpp -- fbr_mom_lanes_sum (csrc/fbr_mom_lanes.h: the producer's wave-wide sum of a column group's rhs moments) on 64
// emulated lanes, for tests/test_gram64_mom_lanes.py (TEST ONLY).  The device runs the same template with register exchanges
// (FbrMomLanesDev, csrc/fbr_gram64.h); here a value is the array of its 64 lanes and an exchange is an index permutation.
#include "../../flobaroid_amd/csrc/fbr_mom_lanes.h"

namespace {
struct V64 {
    double v[64];
};
inline V64 operator+(const V64 &a, const V64 &b)
{
    V64 r;
    for (int i = 0; i < 64; i++) r.v[i] = a.v[i] + b.v[i];
    return r;
}
struct L64 {
    bool b[64];
};
struct Lanes64 {
    static void swap(V64 &a, V64 &b, int bit)
    {
        const V64 a0 = a, b0 = b;
        for (int i = 0; i < 64; i++) {
            a.v[i] = (i & bit) ? b0.v[i ^ bit] : a0.v[i];
            b.v[i] = (i & bit) ? b0.v[i] : a0.v[i ^ bit];
        }
    }
    static V64 get(const V64 &a, int mask)
    {
        V64 r;
        for (int i = 0; i < 64; i++) r.v[i] = a.v[i ^ mask];
        return r;
    }
    void swap32(V64 &a, V64 &b) const { swap(a, b, 32); }
    void swap16(V64 &a, V64 &b) const { swap(a, b, 16); }
    V64 get8(const V64 &a) const { return get(a, 8); }
    V64 get7(const V64 &a) const { return get(a, 7); }
    V64 get2(const V64 &a) const { return get(a, 2); }
    V64 get1(const V64 &a) const { return get(a, 1); }
    V64 live0(const L64 &live, const V64 &a) const
    {
        V64 r;
        for (int i = 0; i < 64; i++) r.v[i] = live.b[i] ? a.v[i] : 0.0;
        return r;
    }
    V64 bit8(const V64 &a, const V64 &b) const
    {
        V64 r;
        for (int i = 0; i < 64; i++) r.v[i] = (i & 8) ? b.v[i] : a.v[i];
        return r;
    }
    V64 zero() const
    {
        V64 r;
        for (int i = 0; i < 64; i++) r.v[i] = 0.0;
        return r;
    }
};

template <int NQ>
void run(const double *v, const L64 &live, double *out)
{
    V64 in[NQ];
    for (int c = 0; c < NQ; c++)
        for (int i = 0; i < 64; i++) in[c].v[i] = v[c * 64 + i];
    const Lanes64 x;
    const V64 r = fbr_mom_lanes_sum<NQ>(in, live, x);
    for (int i = 0; i < 64; i++) out[i] = r.v[i];
}
}  // namespace

extern "C" {
// v [nq][64]: the lanes' values of the nq columns; lanes valid .. 63 are dead.  out [64]: what every lane holds afterwards.
int mom_lanes_sum(int nq, const double *v, int valid, double *out)
{
    L64 live;
    for (int i = 0; i < 64; i++) live.b[i] = i < valid;
    switch (nq) {
    case 1: run<1>(v, live, out); return 0;
    case 2: run<2>(v, live, out); return 0;
    case 3: run<3>(v, live, out); return 0;
    case 4: run<4>(v, live, out); return 0;
    case 6: run<6>(v, live, out); return 0;
    }
    return -1;
}
int mom_lanes_class(int nq, int lane) { return fbr_mom_lanes_class(nq, lane); }
int mom_lane(int pidx, int r) { return fbr_gram64_mom_lane(pidx, r); }
int mom_fric_lane(int pf, int r) { return fbr_gram64_mom_fric_lane(pf, r); }
}
