// The closed-form reach of well-conditioned children (wbvh.hpp wq_fast, wq_fast_eta; DESIGN.md 5.6
// "Closed-form reach") against the bounds it replaces (wq_reach, wq_split, wq_eta), as floats, the way
// wbvh_closest evaluates both: every smin code from the threshold up, every finite L code, qa = W_FAST_Q,
// its next float successors and a grid up to 1, D = 2^-20 .. 2^20 with several mantissas.  Each closed
// form must be >= the function it stands for.  One step below either threshold (and for an L code of 255
// or a NaN qlb) the fast path must not be taken.
// Prints "ok <comparisons> <smallest closed / exact ratio of E, Rlat, Rpar, eta>" or the first violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raytracercpp_amd/csrc/wbvh.hpp"

using namespace rt;

int main()
{
    static_assert(W_FAST_REACH == 1, "built with the closed form on");
    const uint32_t e_ok = W_FAST_S_CODE | (100u << 24);
    const float below = std::nextafter(W_FAST_Q, 0.0f);
    if (!wq_fast_ok(W_FAST_Q, e_ok) || !wq_fast_ok(1.0f, 255u | (254u << 24)) || !wq_fast_ok(W_FAST_Q, W_FAST_S_CODE)) {
        printf("FAIL: the fast path is not taken at its thresholds\n");
        return 1;
    }
    if (wq_fast_ok(below, e_ok) || wq_fast_ok(W_FAST_Q, (W_FAST_S_CODE - 1u) | (100u << 24)) ||
        wq_fast_ok(1.0f, 255u | (255u << 24)) || wq_fast_ok(NAN, e_ok) || wq_fast_ok(-1.0f, e_ok)) {
        printf("FAIL: the fast path is taken below a threshold, without a finite L or for a NaN cosine\n");
        return 1;
    }
    if (!(wq_val_nz(W_FAST_S_CODE, WQ_UNIT) >= W_FAST_S) || wq_val_nz(W_FAST_S_CODE - 1u, WQ_UNIT) >= W_FAST_S) {
        printf("FAIL: W_FAST_S_CODE is not the first code at or above W_FAST_S\n");
        return 1;
    }
    std::vector<float> qs;
    float q = W_FAST_Q;
    for (int i = 0; i < 6; i++, q = std::nextafter(q, 2.0f))
        qs.push_back(q);
    for (int i = 1; i <= 48; i++)
        qs.push_back(W_FAST_Q + (1.0f - W_FAST_Q) * (float)i / 48.0f);
    const float mant[4] = {1.0f, 1.1892071f, 1.5f, 1.9999999f};
    double rmin[4] = {1e300, 1e300, 1e300, 1e300};
    long long n = 0;
    for (uint32_t ks = W_FAST_S_CODE; ks <= 255u; ks++) {
        const float smin = wq_val_nz(ks, WQ_UNIT);
        for (uint32_t kl = 0; kl < 255u; kl++) {
            const float L = wq_val_nz(kl, WQ_LEN);
            for (float qa : qs)
                for (int ex = -20; ex <= 20; ex++)
                    for (int im = 0; im < (ex == 20 ? 1 : 4); im++) {
                        const float D = std::ldexp(mant[im], ex);
                        const WReach wr = wq_reach(qa, smin, L, D);
                        float Rlat, Rpar, fE, fRlat, fRpar;
                        wq_split(wr, L, D, Rlat, Rpar);
                        const float eta = wq_eta(wr, L, D), feta = wq_fast_eta(L, D);
                        wq_fast(L, D, fE, fRlat, fRpar);
                        const float ex4[4] = {wr.E, Rlat, Rpar, eta}, f4[4] = {fE, fRlat, fRpar, feta};
                        for (int k = 0; k < 4; k++) {
                            if (!(f4[k] >= ex4[k])) {
                                printf("FAIL: bound %d: closed form %.9g < %.9g at smin code %u, L code %u, qa %.9g, D %.9g\n", k,
                                       f4[k], ex4[k], ks, kl, qa, D);
                                return 1;
                            }
                            if (ex4[k] > 0.0f)
                                rmin[k] = std::fmin(rmin[k], (double)f4[k] / (double)ex4[k]);
                        }
                        n += 4;
                    }
        }
    }
    printf("ok %lld %.6f %.6f %.6f %.6f\n", n, rmin[0], rmin[1], rmin[2], rmin[3]);
    return 0;
}
