// vrt_step_guard.hpp -- host-only: which arguments of vrt_hip_transmittance_step may reach its kernel.  No HIP, no library: plain C++,
// so that tests/host/step_guard.cpp compiles it on its own.
//
// The kernel restates the reference's Riemann sum (rt.cpp:8-17) with the reference's loop, one lane per sample point s:
//     for (float t = 0; t <= s; t += delta) { one density evaluation per Gaussian }
// in float32.  That loop has arguments it never returns from -- on a GPU a hung queue, not a busy host thread -- and arguments for
// which it returns after hours.  step_guard() refuses both before anything is uploaded or launched.
//
// Why an accepted call ends.  Let S be the largest finite s[k] (samples that are negative, NaN or -inf make zero steps: `t <= s` is
// false at t = 0).  Accepted means delta is a normal float and S < delta * 2^23.  Then for every t the loop reaches, 0 <= t <= S:
//     ulp(t) <= t * 2^-23 <= S * 2^-23 < delta,   so t + delta >= t + ulp(t), which is a float: the rounded sum is > t.
// t grows strictly with every step.  More than that: t + delta <= S + delta, so the rounding error of the sum is at most
// e = ulp(S + delta) / 2 <= delta * (1 + 2^-23) / 2, every step advances t by at least delta - e > 0, t_k >= k (delta - e), and the loop
// makes at most floor(S / (delta - e)) + 1 iterations -- `steps` below.  (delta * 2^23 and everything else here is computed in double,
// where it is exact.)  s = +inf fails the same test for every delta; it is named separately for the message.
// A delta below FLT_MIN is refused because a device that flushes subnormals turns `t += delta` into `t += 0`.
//
// The work cap.  A lane evaluates ceil(S / delta) * max(n, 1) densities one after the other (n = Gaussians of the scene), and the call
// returns when its slowest lane does.  A density term is an exact divide, an accurate exp and a dozen multiply-adds, each waiting for the
// one before: a call with a single sample point is one wave with nothing to hide that latency behind.  The only figure there is: a call
// of 2^22 steps over 5 Gaussians (2.1e7 terms) took about 2.5 s on an MI355X, some 120 ns per term -- three times the 40 cycles
// profiles/r03_erf_term_ubench.txt gives for the comparable erf term at full issue rate.  2^23 terms are then about a second: the most a
// cross-check of a closed form may hold a queue that frames share, and 1,700 times what the reference's own use needs
// (tests/transmittance.cpp: 1,600 steps of 0.01 over 3 Gaussians).  max(n, 1): an empty scene still walks its steps.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace vrtk {

enum StepRefusal {
    STEP_ACCEPT = 0,
    STEP_REFUSE_DELTA,    // delta is not a normal positive float (0, negative, NaN, subnormal)
    STEP_REFUSE_INFINITE, // some s[k] is +inf: `t <= s` is true for every t
    STEP_REFUSE_STALL,    // max finite s[k] >= delta * 2^23: t + delta rounds back to t before t reaches s
    STEP_REFUSE_WORK,     // ceil(max_s / delta) * max(n, 1) exceeds STEP_WORK_CAP
};
constexpr uint64_t STEP_WORK_CAP = (uint64_t)1 << 23; // density evaluations of one lane; see above

struct StepGuard {
    int refusal;    // a StepRefusal
    uint64_t steps; // accepted: no sample point makes more loop iterations than this (0: none makes any)
    uint64_t work;  // accepted: ceil(max_s / delta) * max(n, 1)
};

inline double step_ulp32(double x) // ulp of the float32 binade that holds x > 0 (FLT_MIN's for anything below it)
{
    int e;
    std::frexp(x, &e); // x = m 2^e, 0.5 <= m < 1
    return std::ldexp(1.0, (e < -125 ? -125 : e) - 24);
}

inline StepGuard step_guard(const float *s, size_t ns, float delta, uint32_t n_gaussians)
{
    StepGuard g = { STEP_ACCEPT, 0, 0 };
    if (!(delta >= FLT_MIN)) { g.refusal = STEP_REFUSE_DELTA; return g; }
    bool any = false;
    double S = 0.0;
    for (size_t k = 0; k < ns; ++k) {
        const float v = s[k];
        if (!(v >= 0.f)) continue; // negative, -inf, NaN: zero steps
        if (std::isinf(v)) { g.refusal = STEP_REFUSE_INFINITE; return g; }
        any = true;
        if ((double)v > S) S = v;
    }
    if (!any) return g;
    const double d = delta;
    if (S >= d * 8388608.0) { g.refusal = STEP_REFUSE_STALL; return g; }
    const double work = std::ceil(S / d) * (double)(n_gaussians ? n_gaussians : 1u); // < 2^23 * 2^32: exact in double
    if (work > (double)STEP_WORK_CAP) { g.refusal = STEP_REFUSE_WORK; return g; }
    const double e = 0.5 * step_ulp32(S + d);
    g.steps = (uint64_t)std::floor(S / (d - e)) + 1;
    g.work = (uint64_t)work;
    return g;
}

inline const char *step_refusal_message(int refusal)
{
    switch (refusal) {
    case STEP_REFUSE_DELTA: return "transmittance_step: delta must be a normal positive float (at least FLT_MIN)";
    case STEP_REFUSE_INFINITE: return "transmittance_step: a sample point is +inf: the step loop would never end";
    case STEP_REFUSE_STALL:
        return "transmittance_step: the largest sample point is at least delta * 2^23: t + delta would round back to t and the step loop never end";
    case STEP_REFUSE_WORK: return "transmittance_step: ceil(max s / delta) * max(n, 1) exceeds 2^23 density evaluations in one lane";
    default: return "";
    }
}

} // namespace vrtk
