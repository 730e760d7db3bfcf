// vrt_ray_grad.hpp -- what the derivative kernels of the ray bundles share: vrt_ray_grad_kernel.hip (d radiance / d Gaussians) and
// vrt_ray_trans_grad_kernel.hip (d transmittance / d Gaussians and samples, d depth / d Gaussians and levels), vrt_ray_gn_diag_kernel.hip
// (the diagonal of J^T W J of the radiance) -- and, of grad_gauss, the
// list walk and grad_acc's layout, vrt_ray_tangent_kernel.hip and vrt_ray_trans_tangent_kernel.hip (forward mode: J . v of the radiance, and
// of the transmittance and the depth).  One text each, for these
// translation units and for the short and the long kernel of each:
//   grad_gauss        one Gaussian against one ray with the compensated c = mu - o and mubar = c . n that keep d / d mu accurate: the same
//                     (ray, Gaussian) gives the same A, c_perp, d2 and Erf(-mubar r) in either kind of gradient
//   grad_deal         one weight dealt to one absorber: P, Q, R
//   grad_row, _w      the row segment (d mu xyz, d sigma, d magnitude) from M, the coefficient of n and the sigma sum; with the terms in W
//   grad_deposit      a row segment into the caller's table, wave-summed where every lane names the same row
//   GradSink          where a row segment goes: added to the table, or -- ORDERED -- stored in a record; the record rules and the guard of a ray's range
//   grad_ray_add, _w, grad_ray_store   the same segment's share of the RAY's row (d origin, d direction), and the row's two stores
//   LaneList, grad_acc, grad_walk_begin / _next, grad_flush_short   lane = ray: a lane's list, the three running sums per list position and lane in LDS, the walk of a
//                     lane's list with the next entry's rows loaded one iteration ahead, and every position to the sink once
//   grad_emitter_place, grad_emitter, grad_pass1, grad_pass2    the radiance gradient's emitter set-up, an emitter's weights and the bodies of its two pair loops
//   grad_spread, gn_pass2, gn_rows_squared   the Gauss-Newton diagonal (vrt_ray_gn_diag_kernel.hip): grad_deal's sums spread over the four channels by the
//                     emitter's albedo, pass 2 for the four rows at once, and a complete position's rows squared, weighted and summed
//   trans_grad_x, trans_grad_live   the transmittance derivatives' x_kj and which samples count (depth mode: finite depths > 0)
//   TanRay, tangent_ray, TanGauss, tangent_gauss, tangent_row_load / _uload   forward mode: a direction's ray row and tangent row to three
//                     scalars per (ray, kept Gaussian)
#pragma once
#include "vrt_ray_cull.hpp"

namespace vrtk {

constexpr float ERF_SLOPE = 1.1283791670955126f; // 2 / sqrt(pi): Erf'(x) = ERF_SLOPE exp(-x^2)
constexpr int GRAD_STRIDE = VRT_HIP_GRAD_STRIDE; // floats per row of the caller's table

// a - b as an unevaluated sum hi + lo, exactly (Knuth's two-sum on a and -b)
__device__ __forceinline__ void exact_diff(float a, float b, float &hi, float &lo)
{
    hi = sub_ref(a, b);
    const float bb = sub_ref(hi, a);
    lo = sub_ref(sub_ref(a, sub_ref(hi, bb)), add_ref(b, bb));
}

// One Gaussian against one ray, as both passes and the last walk need it.  d2 is formed from c_perp = c - mubar n itself, not as
// |c|^2 - mubar^2: the vector is needed anyway and its norm has no cancellation.  c = mu - o keeps the low part its rounding drops: the
// exponent d2 / (2 sigma^2) of a small Gaussian far from the origin otherwise carries ulp(|c|) |c_perp| / sigma^2 of error, 1e-4 of a
// row's every entry in the grid scene seen from four units away (a rounding error of mubar only moves c_perp along n: second order).  `on` = false (a lane past the end of its list):
// a harmless row takes the place of whatever was loaded, and the weights are exact zeros.
struct GradGauss {
    float mubar, d2, px, py, pz; // c . n, |c_perp|^2, c_perp
    float r, inv_s, inv_s2;      // 1 / (sqrt2 sigma), 1 / sigma, 1 / sigma^2
    float A, Am, Ar;             // A_j, A_j / m_j (formed without m_j), A_j C r_j
    float m, E;                  // mubar r, Erf(-mubar r)
};
template <int EXP, int ERF>
__device__ __forceinline__ GradGauss grad_gauss(const ErfEval<ERF> &erf, float4 ms, float4 b, bool on, const LaneRay &ray)
{
    if (!on) { ms = make_float4(ray.ox, ray.oy, ray.oz, 1.f); b = make_float4(0.70710678f, 0.5f, 0.f, 0.f); }
    GradGauss q;
    float cx, cy, cz, lx, ly, lz;
    exact_diff(ms.x, ray.ox, cx, lx); exact_diff(ms.y, ray.oy, cy, ly); exact_diff(ms.z, ray.oz, cz, lz);
    // mubar = c . n as hi + lo (products split by fma, sums by two-sum, the low part of c included): a rounding error of mubar moves
    // c_perp along n -- second order in d2, but first order in a component of c_perp that is small against |c| |n's component|
    const float p1 = mul_ref(cx, ray.nx), p2 = mul_ref(cy, ray.ny), p3 = mul_ref(cz, ray.nz);
    const float e1 = __builtin_fmaf(cx, ray.nx, -p1), e2 = __builtin_fmaf(cy, ray.ny, -p2), e3 = __builtin_fmaf(cz, ray.nz, -p3);
    float s12, r12, s123, r123;
    exact_diff(p1, -p2, s12, r12);
    exact_diff(s12, -p3, s123, r123);
    const float tail = add_ref(add_ref(add_ref(add_ref(e1, e2), e3), add_ref(r12, r123)), dot3_ref(lx, ly, lz, ray.nx, ray.ny, ray.nz));
    q.mubar = add_ref(s123, tail);
    const float mlo = add_ref(sub_ref(s123, q.mubar), tail);
    q.px = add_ref(__builtin_fmaf(-mlo, ray.nx, __builtin_fmaf(-q.mubar, ray.nx, cx)), lx);
    q.py = add_ref(__builtin_fmaf(-mlo, ray.ny, __builtin_fmaf(-q.mubar, ray.ny, cy)), ly);
    q.pz = add_ref(__builtin_fmaf(-mlo, ray.nz, __builtin_fmaf(-q.mubar, ray.nz, cz)), lz);
    q.d2 = dot3_ref(q.px, q.py, q.pz, q.px, q.py, q.pz);
    const float ex = vexp<EXP>(-(q.d2 * b.y));
    q.r = b.x; q.inv_s = b.x * SQRT_2; q.inv_s2 = 2.f * b.y;
    q.A = b.z * ex;
    q.Am = on ? (INV_SQRT_2_PI * ms.w) * ex : 0.f;
    q.Ar = q.A * ERF_SLOPE * b.x;
    q.m = q.mubar * b.x;
    q.E = erf(-q.m);
    return q;
}

// NV values per lane for columns col0.. of row idx of the caller's table; `on`: this lane has something to add.  The whole wave calls
// this.  When every lane that is on names the same row, the values are summed over the wave and lanes 0..NV-1 add one segment.
template <int NV>
__device__ __forceinline__ void grad_deposit(float *table, uint32_t idx, bool on, const float (&v)[NV], uint32_t col0, uint32_t lane)
{
    const unsigned long long mask = __ballot(on);
    if (mask == 0ull) return;
    const uint32_t first = lane_value_u32(idx, (uint32_t)__builtin_ctzll(mask));
    const bool shared = __ballot(on && idx == first) == mask && (mask & (mask - 1ull)) != 0ull; // one row, more than one adder
    if (shared) {
        float mine = 0.f;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const float s = wave_sum(on ? v[c] : 0.f);
            if (lane == (uint32_t)c) mine = s;
        }
        if (lane < (uint32_t)NV) atomicAdd(&table[(size_t)first * GRAD_STRIDE + col0 + lane], mine);
    } else if (on) {
#pragma unroll
        for (int c = 0; c < NV; ++c) atomicAdd(&table[(size_t)idx * GRAD_STRIDE + col0 + c], v[c]);
    }
}

// ---- the table sink: where a row segment goes when it leaves a kernel ----
// The only text that knows whether a segment is ADDED to the caller's table P.grad (float atomics: the sums depend on their arrival
// order) or -- ORDERED (vrt_hip_set_grad_ordered) -- STORED in a record that vrt_grad_ordered_kernel.hip sums behind the kernel.  A kernel
// builds one sink, tells it the ray (short_ray, long_ray: ORDERED, the guard of the ray's range) and hands it every segment once.
// A record is (Gaussian index, ray id, GRAD_ORD_COLS floats = the table's columns 0..8) at a place of its ray's own range
// [ord_base[r], ord_base[r] + ord_count[r]); the kernels name it by that place.  The record rules, kept here and nowhere else:
//   - every cell of a record is written by ONE thread, which may read back its own earlier store;
//   - a thread's first write to a cell is a store, every later one (`first` = false) an add onto it;
//   - the first write that OPENS a record (GRAD_OPEN, not GRAD_STORE) stores its name behind the segment, and zeros to the albedo columns
//     where no segment of the kernel writes them (zero_albedo: the transmittance gradient): columns nobody computes are stored as 0.
// Which thread owns which record, and when a write is its first, is the kernel's to say.
enum GradFirst { GRAD_STORE, GRAD_OPEN };
template <bool ORDERED>
struct GradSink {
    const RayArgs *Pp;
    bool zero_albedo; // ORDERED: GRAD_OPEN stores zeros to columns 0..3
    uint64_t r, base; // ORDERED, set by short_ray / long_ray: the ray and the first record of its range,
    bool admits;      // and whether the guard lets this lane's records be stored (a lane of the short kernels)
    __device__ __forceinline__ GradSink(const RayArgs *args, bool zeros) : Pp(args), zero_albedo(zeros) {}

    // is there a table at all?  Wave-uniform.  ORDERED: always (the launch refuses a call without one).
    __device__ __forceinline__ bool table() const { return ORDERED || Pp->grad != nullptr; }
    // is a segment to be formed?  Without RAYS no test: the radiance gradient has its table by contract, and the transmittance gradient,
    // which may be asked for grad_s alone, gets here only behind table().
    template <bool RAYS>
    __device__ __forceinline__ bool wanted() const { return !RAYS || table(); }

    // A lane of the short kernels behind ray_short_begin: its ray's range, and the guard.
    __device__ __forceinline__ void short_ray(const ShortRay &R)
    {
        if constexpr (ORDERED) {
            r = R.rc;
            base = Pp->ord_base[R.rc];
            admits = R.writes && R.nl == Pp->ord_len[R.rc];
            if (R.writes && !admits) mismatch(R.rc, 0u, 1u);
        }
    }
    // The wave of a long kernel behind ray_long_next, `per_gauss` records per kept Gaussian: the ray's range, and the guard -- the re-cull
    // gives the counted length, and the range is a long ray's.  false: the mismatch is filed, skip the ray.
    __device__ __forceinline__ bool long_ray(uint64_t ray_id, uint32_t n, uint32_t per_gauss, uint32_t lane)
    {
        if constexpr (ORDERED) {
            if (n != Pp->ord_len[ray_id] || Pp->ord_count[ray_id] != (uint64_t)per_gauss * n) { mismatch(ray_id, lane, 64u); return false; }
            r = ray_id;
            base = Pp->ord_base[ray_id];
        }
        return true;
    }

    // One thread's segment: NV values for columns col0.. of Gaussian idx -- added to its row, or written to record `rec` of the ray's range
    template <int NV>
    __device__ __forceinline__ void put(uint64_t rec, uint32_t idx, uint32_t col0, const float (&v)[NV], GradFirst how, bool first = true) const
    {
        if constexpr (ORDERED) {
            float *row = Pp->ord_rows + (base + rec) * (uint64_t)GRAD_ORD_COLS;
            if (first) {
                if (how == GRAD_OPEN && zero_albedo) { row[0] = 0.f; row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; }
#pragma unroll
                for (int c = 0; c < NV; ++c) row[col0 + c] = v[c];
                if (how == GRAD_OPEN) name(base + rec, idx);
            } else {
#pragma unroll
                for (int c = 0; c < NV; ++c) row[col0 + c] = row[col0 + c] + v[c];
            }
        } else {
            float *row = Pp->grad + (size_t)idx * GRAD_STRIDE + col0;
#pragma unroll
            for (int c = 0; c < NV; ++c) atomicAdd(row + c, v[c]);
        }
    }
    // The short kernels' deposit, called by the whole wave; `on`: this lane has something.  Added through grad_deposit, wave-summed where
    // every lane names one row -- or one record per lane, a first write, no sum across lanes: a record holds its own ray's share.
    template <int NV>
    __device__ __forceinline__ void deposit(uint64_t rec, uint32_t idx, bool on, const float (&v)[NV], uint32_t col0, uint32_t lane, GradFirst how) const
    {
        if constexpr (ORDERED) {
            if (on && admits) put<NV>(rec, idx, col0, v, how);
        } else
            grad_deposit<NV>(Pp->grad, idx, on, v, col0, lane);
    }
    // The long radiance kernel's absorber segment, called by the whole wave: lanes 0..4 hold one column each in `mine` and add it -- or own
    // columns 4..8 of record `rec` across the rounds, where lanes 5..8 store the zeros of columns 0..3 and lane 9 the name in the first.
    __device__ __forceinline__ void absorber(uint64_t rec, uint32_t idx, float mine, uint32_t lane, bool first) const
    {
        if constexpr (ORDERED) {
            float *row = Pp->ord_rows + (base + rec) * (uint64_t)GRAD_ORD_COLS;
            if (lane < 5u) row[4u + lane] = first ? mine : row[4u + lane] + mine;
            else if (first && lane < 9u) row[lane - 5u] = 0.f;
            else if (first && lane == 9u) name(base + rec, idx);
        } else if (lane < 5u) atomicAdd(&Pp->grad[(size_t)idx * GRAD_STRIDE + 4u + lane], mine);
    }

private:
    __device__ __forceinline__ void name(uint64_t at, uint32_t idx) const { name_as(at, idx, r); }
    __device__ __forceinline__ void name_as(uint64_t at, uint32_t idx, uint64_t ray_id) const
    {
        Pp->ord_gauss[at] = idx;
        Pp->ord_ray[at] = (uint32_t)ray_id;
    }
    // A ray whose list is not as long as the count pass found it names every row of its range a sentinel (key = N: sorted last, read by no
    // segment), touches nothing outside the range and counts one mismatch.  Called by the lanes `lanes` apart that share the ray (1: a lane
    // of the short kernels, 64: the wave of the long ones, `first` = the lane's place among them).
    __device__ __forceinline__ void mismatch(uint64_t ray_id, uint32_t first, uint32_t lanes) const
    {
        const uint64_t range = Pp->ord_base[ray_id], rows = Pp->ord_count[ray_id];
        for (uint64_t k = first; k < rows; k += lanes) name_as(range + k, Pp->S.n, ray_id);
        if (first == 0) atomicAdd(&Pp->ord_words[GRAD_ORD_MISMATCH], 1ull);
    }
};

// One weight w dealt to one absorber at x = x_ikj (or x_kj), E = Erf(-mubar_j r_j): P += w D, Q += w e2, R += w e2 x.  Returns w e2.
template <int EXP, int ERF>
__device__ __forceinline__ float grad_deal(const ErfEval<ERF> &erf, float w, float x, float E, float &P, float &Q, float &R)
{
    const float we = w * exp_neg_sq<EXP>(x);
    P = __builtin_fmaf(w, E - erf(x), P);
    Q += we;
    R = __builtin_fmaf(we, x, R);
    return we;
}

// The row segment of one Gaussian against one ray: d = (d mu xyz, d sigma, d magnitude) from M = d magnitude, the coefficient of n in
// d mu and the sum that joins m M (1 / sigma + d2 / sigma^3) in d sigma.
__device__ __forceinline__ void grad_row(const GradGauss &q, const LaneRay &ray, float mag, float M, float ncoef, float ssum, float (&d)[5])
{
    const float mM = mag * M;
    const float alpha = -mM * q.inv_s2;
    d[0] = __builtin_fmaf(alpha, q.px, ncoef * ray.nx);
    d[1] = __builtin_fmaf(alpha, q.py, ncoef * ray.ny);
    d[2] = __builtin_fmaf(alpha, q.pz, ncoef * ray.nz);
    d[3] = mM * (q.inv_s + q.d2 * q.inv_s * q.inv_s2) + ssum;
    d[4] = M;
}
// ... with the terms in W = the sum of all weights: -A C r e1 W onto the coefficient of n, A C r e1 m sqrt2 W onto d sigma, behind its other terms
template <int EXP>
__device__ __forceinline__ void grad_row_w(const GradGauss &q, const LaneRay &ray, float mag, float M, float ncoef, float ssum, float W, float (&d)[5])
{
    const float ArE = q.Ar * exp_neg_sq<EXP>(q.m);
    grad_row(q, ray, mag, M, __builtin_fmaf(-ArE, W, ncoef), ssum, d);
    d[3] = d[3] + ArE * q.m * SQRT_2 * W;
}

// ---- the ray's own row: d(loss) / d(origin, direction) ----
// Every observable depends on the ray (o, n) through c_j = mu_j - o and n alone, and ray r's share of row j's d mu is a c_perp + b n with
// a = -mag M / sigma^2 (grad_row's alpha) and b the whole coefficient of n.  Hence ("Ray gradients")
//   d / d o = -sum_j (a_j c_perp_j + b_j n)                  (translation invariance)
//   d / d n =  sum_j (b_j - a_j mubar_j) c_perp_j            (tangential: along normalise(n + eps t), t perpendicular to n)
// Both are linear in (M, ncoef): grad_ray_add is called with the arguments of grad_row wherever a row segment is formed, and adds that
// segment's share to six accumulators -- from a, b, mubar and c_perp themselves, not by projecting the finished row.  No atomic add: a
// lane of the short kernels sums its ray's shares in list order, the long kernels finish with one wave_sum per component.
constexpr int RAY_GRAD_STRIDE = VRT_HIP_RAY_GRAD_STRIDE; // floats per ray row: [0..2] d origin, [3] 0, [4..6] d direction, [7] 0
__device__ __forceinline__ void grad_ray_add(const GradGauss &q, const LaneRay &ray, float mag, float M, float ncoef, float (&go)[3], float (&gn)[3])
{
    const float a = -(mag * M) * q.inv_s2;
    const float t = __builtin_fmaf(-a, q.mubar, ncoef);
    go[0] -= __builtin_fmaf(a, q.px, ncoef * ray.nx);
    go[1] -= __builtin_fmaf(a, q.py, ncoef * ray.ny);
    go[2] -= __builtin_fmaf(a, q.pz, ncoef * ray.nz);
    gn[0] = __builtin_fmaf(t, q.px, gn[0]);
    gn[1] = __builtin_fmaf(t, q.py, gn[1]);
    gn[2] = __builtin_fmaf(t, q.pz, gn[2]);
}
// ... with the term in W on the coefficient of n, as grad_row_w
template <int EXP>
__device__ __forceinline__ void grad_ray_add_w(const GradGauss &q, const LaneRay &ray, float mag, float M, float ncoef, float W, float (&go)[3], float (&gn)[3])
{
    grad_ray_add(q, ray, mag, M, __builtin_fmaf(-(q.Ar * exp_neg_sq<EXP>(q.m)), W, ncoef), go, gn);
}
// ray r's row, STORED as two 16-byte stores
__device__ __forceinline__ void grad_ray_store(float *grad_rays, uint64_t r, const float (&go)[3], const float (&gn)[3])
{
    float4 *row = (float4 *)(grad_rays + r * (uint64_t)RAY_GRAD_STRIDE);
    row[0] = make_float4(go[0], go[1], go[2], 0.f);
    row[1] = make_float4(gn[0], gn[1], gn[2], 0.f);
}

// ---- lane = ray (the short kernels) ----

// s_acc: three running sums per list position and lane, [(c * RAY_PL + pos) * 64 + lane]: c = 0 M (d magnitude), 1 the coefficient of n,
// 2 the sigma sum, the last two without their terms in W
__device__ __forceinline__ float &grad_acc(float *s_acc, int c, uint32_t pos, uint32_t lane) { return s_acc[((uint32_t)c * RAY_PL + pos) * 64u + lane]; }

// A lane's list: s_list[k*64 + lane], nl entries; loops over it run to nmax, the longest list of the wave's short rays
struct LaneList {
    const uint32_t *s_list;
    uint32_t lane, nl, nmax;
    __device__ __forceinline__ bool has(uint32_t j) const { return j < nl; }
    __device__ __forceinline__ uint32_t at(uint32_t j) const { return j < nl ? s_list[j * 64 + lane] : 0u; } // past the end: row 0, never used
};

// One walk of a lane's list with the next entry's rows loaded one iteration ahead: grad_walk_begin loads the first entry's rows,
// grad_walk_next hands out position j's grad_gauss (a harmless row with exact zero weights where the list has no position j) and loads
// the rows of position j + 1.  The for (j < nmax) stays with the kernel (profiles/grad_bundle_refactor.md).
struct ListWalk {
    uint32_t lj;
    float4 a, b;
};
__device__ __forceinline__ ListWalk grad_walk_begin(const SceneTables &S, const LaneList &L)
{
    ListWalk w;
    w.lj = L.at(0);
    w.a = S.mu_sig[w.lj]; w.b = S.gB[w.lj];
    return w;
}
template <int EXP, int ERF>
__device__ __forceinline__ GradGauss grad_walk_next(ListWalk &w, const SceneTables &S, const ErfEval<ERF> &erf, const LaneList &L, const LaneRay &ray, uint32_t j)
{
    const float4 ca = w.a, cb = w.b;
    if (j + 1 < L.nmax) {
        w.lj = L.at(j + 1);
        w.a = S.mu_sig[w.lj]; w.b = S.gB[w.lj];
    }
    return grad_gauss<EXP, ERF>(erf, ca, cb, L.has(j), ray);
}

// Every list position to the sink once, now that W is known (position p: record p of the lane's ray, opened here), and -- RAYS -- the same
// segments to the lane's ray row in list order, stored once where the lane `writes`.  With RAYS the table may be missing (wave-uniform:
// no segment is formed); without, it is there, and this is the text the kernels ran before there were ray rows.  The whole wave calls this.
template <int EXP, int ERF, bool RAYS, bool ORDERED>
__device__ __forceinline__ void grad_flush_short(const GradSink<ORDERED> &sink, [[maybe_unused]] float *grad_rays, [[maybe_unused]] uint64_t r,
                                                 [[maybe_unused]] bool writes, const SceneTables &S, const ErfEval<ERF> &erf, const LaneList &L, float *s_acc,
                                                 const LaneRay &ray, float W)
{
    const uint32_t lane = L.lane;
    [[maybe_unused]] float go[3] = { 0.f, 0.f, 0.f }, gn[3] = { 0.f, 0.f, 0.f };
    for (uint32_t p = 0; p < L.nmax; ++p) {
        const bool on = L.has(p); // nl is 0 in a lane without a ray of this kernel
        const uint32_t idx = L.at(p);
        const GradGauss q = grad_gauss<EXP, ERF>(erf, S.mu_sig[idx], S.gB[idx], on, ray);
        const float mag = on ? S.gD[idx].z : 0.f;
        if constexpr (RAYS) {
            if (on) grad_ray_add_w<EXP>(q, ray, mag, grad_acc(s_acc, 0, p, lane), grad_acc(s_acc, 1, p, lane), W, go, gn);
        }
        if (sink.template wanted<RAYS>()) {
            float d[5];
            grad_row_w<EXP>(q, ray, mag, grad_acc(s_acc, 0, p, lane), grad_acc(s_acc, 1, p, lane), grad_acc(s_acc, 2, p, lane), W, d);
            sink.template deposit<5>(p, idx, on, d, 4u, lane, GRAD_OPEN);
        }
    }
    if constexpr (RAYS) {
        if (writes) grad_ray_store(grad_rays, r, go, gn); // a ray that keeps nothing: exact zeros
    }
}

// ---- the radiance gradient's pair loops: EC emitters against one absorber q (per lane in the short kernel, wave-uniform in the long) ----

// where emitter (row ms) sits on the ray: the centre of its five sample points and their spacing; a lane without it gets a harmless one
__device__ __forceinline__ void grad_emitter_place(bool on, float4 ms, const LaneRay &ray, float &mubar, float &sigma)
{
    const float cx = ms.x - ray.ox, cy = ms.y - ray.oy, cz = ms.z - ray.oz;
    mubar = on ? dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz) : 0.f;
    sigma = on ? ms.w : 1.f;
}

// What an emitter contributes once the exponents of its five samples are known: t_k = sigma exp(acc_k - d2 / (2 sigma^2) - k^2 / 2)
// (the ik term of L without m_i), V = sum_k t_k, w_k = G m t_k.
template <int EXP>
__device__ __forceinline__ float grad_emitter(bool on, float sigma, float d2, float inv2s2, float Gm, const float (&acc)[5], float (&w)[5])
{
    float V = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float kf = (float)(k - 4);
        const float t = sigma * vexp<EXP>(acc[k] - d2 * inv2s2 - 0.5f * kf * kf);
        V += t;
        w[k] = on ? Gm * t : 0.f;
    }
    return on ? V : 0.f; // a lane without this emitter: exact zeros, whatever its exponents came to
}

// One emitter's scalar sums p, q, r (what grad_deal makes of w = m t, the weights without their albedo) spread over the four channels by
// the emitter's albedo: the sums of channel c are a_c times the scalar ones (the Gauss-Newton diagonal, vrt_ray_gn_diag_kernel.hip)
__device__ __forceinline__ void grad_spread(const float (&alb)[4], float p, float q, float r, float (&Pc)[4], float (&Qc)[4], float (&Rc)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        Pc[c] = __builtin_fmaf(alb[c], p, Pc[c]);
        Qc[c] = __builtin_fmaf(alb[c], q, Qc[c]);
        Rc[c] = __builtin_fmaf(alb[c], r, Rc[c]);
    }
}

// pass 1: q's term of the exponents of T at the emitters' 5 EC sample points (the radiance kernel's pair loop)
template <int ERF, int EC>
__device__ __forceinline__ void grad_pass1(const ErfEval<ERF> &erf, const GradGauss &q, const float (&e_mubar)[EC], const float (&e_sigma)[EC], float (&acc)[EC][5])
{
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const float base = __builtin_fmaf(e_mubar[e], q.r, -q.m);
        const float step = e_sigma[e] * q.r;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float x = __builtin_fmaf((float)(k - 4), step, base);
            acc[e][k] = __builtin_fmaf(q.A, q.E - erf(x), acc[e][k]);
        }
    }
}

// pass 2: the same pairs again; w_ik dealt to absorber q (P, Q, R) and through w e2 A C r back to the emitters (z, y)
template <int EXP, int ERF, int EC>
__device__ __forceinline__ void grad_pass2(const ErfEval<ERF> &erf, const GradGauss &q, const float (&e_mubar)[EC], const float (&e_sigma)[EC], const float (&w)[EC][5],
                                           float (&z)[EC], float (&y)[EC], float &Pj, float &Qj, float &Rj)
{
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const float base = __builtin_fmaf(e_mubar[e], q.r, -q.m);
        const float step = e_sigma[e] * q.r;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float kf = (float)(k - 4);
            const float t = q.Ar * grad_deal<EXP>(erf, w[e][k], __builtin_fmaf(kf, step, base), q.E, Pj, Qj, Rj);
            z[e] += t;
            y[e] = __builtin_fmaf(kf, t, y[e]);
        }
    }
}

// ---- the Gauss-Newton diagonal (vrt_ray_gn_diag_kernel.hip): the four Jacobian rows of a (ray, kept Gaussian), squared per ray ----
// (GN_SUMS of vrt_kernels.h: the running sums per (ray, list position))

// pass 2 for all four channels at once: w = m t (no albedo, no g); per emitter the scalar sums of grad_deal are formed once and spread by
// its albedo (grad_spread), z and y stay scalar (the channel's are a_c z, a_c y).  D, e2, the Erf and both Exps are paid once.
template <int EXP, int ERF, int EC>
__device__ __forceinline__ void gn_pass2(const ErfEval<ERF> &erf, const GradGauss &q, const float (&e_mubar)[EC], const float (&e_sigma)[EC], const float (&w)[EC][5],
                                         const float (&alb)[EC][4], float (&z)[EC], float (&y)[EC], float (&Pc)[4], float (&Qc)[4], float (&Rc)[4])
{
#pragma unroll
    for (int e = 0; e < EC; ++e) {
        const float base = __builtin_fmaf(e_mubar[e], q.r, -q.m);
        const float step = e_sigma[e] * q.r;
        float p = 0.f, qq = 0.f, r = 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float kf = (float)(k - 4);
            const float t = q.Ar * grad_deal<EXP>(erf, w[e][k], __builtin_fmaf(kf, step, base), q.E, p, qq, r);
            z[e] += t;
            y[e] = __builtin_fmaf(kf, t, y[e]);
        }
        grad_spread(alb[e], p, qq, r, Pc, Qc, Rc);
    }
}

// A complete position: grad_row_w per channel as it stands, each row squared and weighted, d[i] = sum_c wt_c row_c[i]^2 (columns 4..8)
template <int EXP>
__device__ __forceinline__ void gn_rows_squared(const GradGauss &q, const LaneRay &ray, float mag, const float (&sums)[GN_SUMS], const float (&W)[4], const float (&wt)[4],
                                                float (&d)[5])
{
#pragma unroll
    for (int i = 0; i < 5; ++i) d[i] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float row[5];
        grad_row_w<EXP>(q, ray, mag, sums[3 * c], sums[3 * c + 1], sums[3 * c + 2], W[c], row);
#pragma unroll
        for (int i = 0; i < 5; ++i) d[i] = __builtin_fmaf(wt[c] * row[i], row[i], d[i]);
    }
}

// ---- what the transmittance derivative units share (vrt_ray_trans_grad_kernel.hip, vrt_ray_trans_tangent_kernel.hip) ----

// x_kj = (s_k - mubar_j) r_j, the difference first: s r - m would round at the size of m = mubar r (20 and more for a narrow Gaussian a unit
// away), and e2 = exp(-x^2) passes an error dx on as 2 |x| dx -- 4e-5 of a far sample's addends on the grid scene, against 5e-6 this way.
__device__ __forceinline__ float trans_grad_x(float s, const GradGauss &q) { return (s - q.mubar) * q.r; }

// is sample (s, g) live: g_k != 0, and in depth mode s_k finite and > 0 (a depth bundle's +inf, 0 and NaN results are not).  The kernels
// carry a sample that is not as g = 0 at s = 0 (finite arithmetic, weight exactly 0).  Forward mode has no g: it asks with g = 1.
__device__ __forceinline__ bool trans_grad_live(bool depth_mode, float s, float g)
{
    return g != 0.f && (!depth_mode || (s > 0.f && s < __builtin_inff()));
}

// ---- forward mode (vrt_ray_tangent_kernel.hip, vrt_ray_trans_tangent_kernel.hip): a direction's rows to scalars per (ray, kept Gaussian) ----

// The ray's own tangent: d origin and d direction.  The direction tangent enters through c_perp_j . t alone (tangent_gauss), and c_perp is
// perpendicular to n: a component of t along n -- which does not move normalise(n + eps t) -- drops out there, to rounding, exactly as the
// gradient kernels' ray row sum_j (..) c_perp_j is perpendicular to n to rounding.  No projection of t: J . v is the transpose of that row
// term for term, whatever the float32 direction's length is off 1 by.
struct TanRay { float ox, oy, oz, nx, ny, nz; };
__device__ __forceinline__ TanRay tangent_ray(const float *ray_tangent, uint64_t r)
{
    TanRay t = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    if (ray_tangent) { // wave-uniform
        const float4 *row = (const float4 *)(ray_tangent + r * (uint64_t)RAY_GRAD_STRIDE);
        const float4 a = row[0], b = row[1]; // .w of either is never used
        t.ox = a.x; t.oy = a.y; t.oz = a.z;
        t.nx = b.x; t.ny = b.y; t.nz = b.z;
    }
    return t;
}

// What the pair loop needs of one Gaussian's tangent row against one ray
struct TanGauss { float dmubar, u, ds; };
// q: grad_gauss of the same (ray, Gaussian); ms_t = (d mu xyz, d sigma), dm = d magnitude; `on` = false: exact zeros, whatever was loaded
__device__ __forceinline__ TanGauss tangent_gauss(const GradGauss &q, const LaneRay &ray, const TanRay &tr, float mag, float4 ms_t, float dm, bool on)
{
    if (!on) { ms_t = make_float4(0.f, 0.f, 0.f, 0.f); dm = 0.f; }
    const float cx = ms_t.x - tr.ox, cy = ms_t.y - tr.oy, cz = ms_t.z - tr.oz;
    const float cn = dot3_ref(q.px, q.py, q.pz, tr.nx, tr.ny, tr.nz);
    TanGauss g;
    g.dmubar = on ? dot3_ref(cx, cy, cz, ray.nx, ray.ny, ray.nz) + cn : 0.f;
    const float dd2 = 2.f * __builtin_fmaf(-q.mubar, cn, dot3_ref(q.px, q.py, q.pz, cx, cy, cz));
    g.ds = ms_t.w * q.inv_s;
    const float dlog = __builtin_fmaf(q.d2 * q.inv_s2, g.ds, __builtin_fmaf(-0.5f * dd2, q.inv_s2, g.ds));
    g.u = on ? __builtin_fmaf(mag, dlog, dm) : 0.f;
    if (!on) g.ds = 0.f;
    return g;
}
// columns 4..11 of row idx of the tangent table: (d mu xyz, d sigma) and d magnitude; columns 9..11 come along and are dropped
__device__ __forceinline__ void tangent_row_load(const float *table, uint32_t idx, float4 &ms_t, float &dm)
{
    const float4 *row = (const float4 *)(table + (size_t)idx * GRAD_STRIDE);
    ms_t = row[1];
    dm = row[2].x;
}
__device__ __forceinline__ void tangent_row_uload(const float *table, uint32_t idx, float4 &ms_t, float &dm)
{
    ms_t = uload((const float4 *)table, 3u * idx + 1u);
    dm = uload((const float4 *)table, 3u * idx + 2u).x;
}

// ---- the launch: a bundle's run-time list source (RayListSource) as the constant I.value of a generic callable f(I), and with RAYS as
// the constants I.value, R.value of f(I, R) ----
template <class F>
inline void grad_dispatch_source(int src, F &&f)
{
    if (src == RAY_LIST_PLAN) f(std::integral_constant<int, RAY_LIST_PLAN>());
    else if (src == RAY_LIST_INDEX) f(std::integral_constant<int, RAY_LIST_INDEX>());
    else f(std::integral_constant<int, RAY_LIST_CHUNKS>());
}
template <class F>
inline void grad_dispatch_source_rays(int src, bool rays, F &&f)
{
    grad_dispatch_source(src, [&](auto I) {
        if (rays) f(I, std::true_type());
        else f(I, std::false_type());
    });
}

} // namespace vrtk
