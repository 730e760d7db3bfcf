// vrt_hip_diag.cpp -- diagnostics of libvrt_hip.so: per-render statistics, the kernel timing ring and the kernel
// timelines (VRT_HIP_TIMELINE).
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#include "vrt_hip_ctx.hpp"

// The event ring of vrt_hip_enable_kernel_timing: 4 events per timed frame (vrt_hip_ctx::tev).
int ensure_timing_ring(vrt_hip_ctx *c)
{
    if (!c->tev.empty()) return VRT_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->tev.resize(4 * vrt_hip_ctx::TIMING_RING);
    for (auto &e : c->tev) HIPCHK(c, hipEventCreate(&e));
    return VRT_HIP_OK;
}

// vrt_hip_render with stats on: the counters its kernels summed (d_stats) into vrt_hip_stats
int read_stats(vrt_hip_ctx *c)
{
    using namespace vrtk;
    unsigned long long st[STAT_WORDS];
    HIPCHK(c, hipMemcpy(st, c->d_stats.p, sizeof st, hipMemcpyDeviceToHost));
    c->last.table_nodes = st[STAT_TABLE_NODES]; c->last.table_retries = st[STAT_TABLE_RETRIES]; c->last.table_skips = st[STAT_TABLE_SKIPS];
    c->last.table_declined = st[STAT_TABLE_DECLINED]; c->last.table_coarser = st[STAT_TABLE_COARSER]; c->last.table_empty = st[STAT_TABLE_EMPTY];
    for (int k = 0; k < 8; ++k) c->last.table_phase_ticks[k] = st[STAT_TABLE_PHASE + k];
    if (c->tune.table_diag && st[STAT_TABLE_BLOCKS]) // the table phase split by every wave's clock: staging | node loops | waiting at the chunk barriers
        fprintf(stderr, "[vrt_hip] table kernel, us per block of its table phase (%.1f): node loops %.1f, waiting at the chunk barriers %.1f, staging the rest (mean over the 16 waves)\n",
                st[STAT_TABLE_PHASE + 5] * 0.01 / st[STAT_TABLE_BLOCKS], st[STAT_TABLE_NODE_TICKS] * 0.01 / 16 / st[STAT_TABLE_BLOCKS],
                st[STAT_TABLE_WAIT_TICKS] * 0.01 / 16 / st[STAT_TABLE_BLOCKS]);
    c->last.lane_pairs = st[STAT_LANE_PAIRS];
    c->last.dense_visits_full = st[STAT_DENSE_VISITS_FULL]; c->last.dense_visits_zero = st[STAT_DENSE_VISITS_ZERO]; c->last.dense_visits_common = st[STAT_DENSE_VISITS_COMMON];
    c->last.dense_busy_frac = (st[STAT_DENSE_WORKGROUPS] && st[STAT_DENSE_T_LAST] > st[STAT_DENSE_T_FIRST])
                                  ? (double)st[STAT_DENSE_BUSY_TICKS] / ((double)st[STAT_DENSE_WORKGROUPS] * (double)(st[STAT_DENSE_T_LAST] - st[STAT_DENSE_T_FIRST]))
                                  : 0.0;
    c->last.shaded_blocks = st[STAT_SHADED_BLOCKS] + st[STAT_DENSE_BLOCKS];
    c->last.dense_blocks = st[STAT_DENSE_BLOCKS];
    c->last.table_blocks = st[STAT_TABLE_BLOCKS];
    c->last.list_entries = st[STAT_BLOCK_CANDIDATES]; c->last.tile_entries = st[STAT_TILE_ENTRIES]; c->last.overflow_blocks = st[STAT_DENSE_OVER_DCAP];
    c->last.lane_entries = st[STAT_LANE_ENTRIES]; c->last.lane_max_entries = st[STAT_LANE_MAX_ENTRIES];
    return VRT_HIP_OK;
}

// VRT_HIP_TIMELINE: where the one-wave kernel's time goes (wall_clock64 ticks are 10 ns), printed by vrt_hip_render()
void print_timeline(vrt_hip_ctx *c)
{
    if (c->timeline_tiles) {
        std::vector<unsigned long long> tt(c->timeline_tiles * 8);
        if (hipMemcpy(tt.data(), c->d_timeline_lists.p, tt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
            unsigned long long a = ~0ull, b = 0;
            double ph[5] = {0, 0, 0, 0, 0}, s_start = 0, n = 0, worst = 0, wph[5] = {0, 0, 0, 0, 0};
            size_t worst_i = 0;
            for (size_t i = 0; i < c->timeline_tiles; ++i) {
                const unsigned long long *e = &tt[8 * i];
                if (!e[4]) continue;
                a = std::min(a, e[0]); b = std::max(b, e[5] ? e[5] : e[4]);
            }
            for (size_t i = 0; i < c->timeline_tiles; ++i) {
                const unsigned long long *e = &tt[8 * i];
                if (!e[4]) continue;
                n += 1; s_start += (double)(e[0] - a);
                for (int k = 0; k < 5; ++k) ph[k] += (e[k + 1] >= e[k] && e[k + 1]) ? (double)(e[k + 1] - e[k]) : 0.0;
                const double dur = (double)((e[5] ? e[5] : e[4]) - e[0]);
                if (dur > worst) {
                    worst = dur; worst_i = i;
                    for (int k = 0; k < 5; ++k) wph[k] = (e[k + 1] >= e[k] && e[k + 1]) ? (double)(e[k + 1] - e[k]) : 0.0;
                }
            }
            if (n > 0)
                fprintf(stderr, "[vrt_hip] list kernel timeline: %.0f tiles, span %.2f us, mean start %.2f us; per tile: cone %.2f us, "
                                "level 1 %.2f us, level 2 %.2f us, filing %.2f us, clear %.2f us\n", n, (b - a) * 0.01, s_start / n * 0.01,
                        ph[0] / n * 0.01, ph[1] / n * 0.01, ph[2] / n * 0.01, ph[3] / n * 0.01, ph[4] / n * 0.01);
            if (n > 0)
                fprintf(stderr, "[vrt_hip]   slowest tile %zu: %.2f us = %.2f + %.2f + %.2f + %.2f + %.2f\n", worst_i, worst * 0.01,
                        wph[0] * 0.01, wph[1] * 0.01, wph[2] * 0.01, wph[3] * 0.01, wph[4] * 0.01);
        }
    }
    std::vector<unsigned long long> tl(c->timeline_items * 5);
    if (hipMemcpy(tl.data(), c->d_timeline.p, tl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return;
    unsigned long long t0 = ~0ull, t1 = 0;
    double n = 0, s_start = 0, s_end = 0, p0 = 0, p1 = 0, p2 = 0;
    for (size_t i = 0; i < c->timeline_items; ++i)
        if (tl[5 * i + 3]) { t0 = std::min(t0, tl[5 * i]); t1 = std::max(t1, tl[5 * i + 3]); }
    std::vector<unsigned> starts(64, 0), ends(64, 0);
    std::map<uint32_t, std::pair<int, double>> per_simd; // blocks, last end (us)
    std::map<uint32_t, int> per_cu;
    for (size_t i = 0; i < c->timeline_items; ++i) {
        const unsigned long long *e = &tl[5 * i];
        if (!e[3]) continue;
        {   // gfx9 HW_ID: simd [5:4], cu [11:8], sh [12], se [15:13]; XCC_ID [3:0]
            const uint32_t hw = (uint32_t)e[4], xcc = (uint32_t)(e[4] >> 32) & 15u;
            const uint32_t cu = (xcc << 8) | (((hw >> 13) & 7u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u);
            const uint32_t simd = (cu << 2) | ((hw >> 4) & 3u);
            auto &a = per_simd[simd]; a.first += 1; a.second = std::max(a.second, (double)(e[3] - t0) * 0.01);
            per_cu[cu] += 1;
        }
        n += 1; s_start += (double)(e[0] - t0); s_end += (double)(e[3] - t0);
        p0 += (double)(e[1] - e[0]); p1 += (double)(e[2] - e[1]); p2 += (double)(e[3] - e[2]);
        const double span = (double)(t1 - t0) + 1;
        ++starts[(size_t)((e[0] - t0) * 64.0 / span)]; ++ends[(size_t)((e[3] - t0) * 64.0 / span)];
    }
    if (n == 0) return;
    if (!c->tune.timeline_csv.empty()) { // raw stamps for offline analysis
        if (FILE *f = fopen(c->tune.timeline_csv.c_str(), "w")) {
            fprintf(f, "item,t0,t1,t2,t3,hw_id,xcc_id,nmax\n");
            for (size_t i = 0; i < c->timeline_items; ++i) {
                const unsigned long long *e = &tl[5 * i];
                if (e[3]) fprintf(f, "%zu,%llu,%llu,%llu,%llu,%u,%u,%u\n", i, e[0] - t0, e[1] - t0, e[2] - t0, e[3] - t0, (unsigned)e[4], (unsigned)(e[4] >> 32) & 0xFFFFu, (unsigned)(e[4] >> 48));
            }
            fclose(f);
        }
    }
    fprintf(stderr, "[vrt_hip] one-wave kernel timeline: %.0f blocks, span %.2f us, mean start %.2f us, mean end %.2f us; per block: "
                    "block cull %.2f us, lane lists %.2f us, shade+store %.2f us\n[vrt_hip]   running blocks per 1/64 of the span:",
            n, (t1 - t0) * 0.01, s_start / n * 0.01, s_end / n * 0.01, p0 / n * 0.01, p1 / n * 0.01, p2 / n * 0.01);
    long running = 0;
    for (int b = 0; b < 64; ++b) { running += starts[b]; fprintf(stderr, " %ld", running); running -= ends[b]; }
    fprintf(stderr, "\n");
    std::map<int, std::pair<int, double>> by_count; // blocks on a SIMD -> (SIMDs, mean last end)
    for (auto &kv : per_simd) { auto &b = by_count[kv.second.first]; b.first += 1; b.second += kv.second.second; }
    fprintf(stderr, "[vrt_hip]   %zu CUs, %zu SIMDs seen; blocks per SIMD -> SIMDs (mean time of their last block end):", per_cu.size(), per_simd.size());
    for (auto &kv : by_count) fprintf(stderr, "  %d -> %d (%.1f us)", kv.first, kv.second.first, kv.second.second / kv.second.first);
    std::map<int, int> cu_hist;
    for (auto &kv : per_cu) cu_hist[kv.second] += 1;
    fprintf(stderr, "\n[vrt_hip]   blocks per CU -> CUs:");
    for (auto &kv : cu_hist) fprintf(stderr, "  %d -> %d", kv.first, kv.second);
    fprintf(stderr, "\n");
}

extern "C" {

int vrt_hip_enable_stats(vrt_hip_ctx *c, int on)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    c->stats_on = on != 0;
    return VRT_HIP_OK;
}

int vrt_hip_enable_kernel_timing(vrt_hip_ctx *c, int on)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    c->timing_on = on != 0;
    c->timing_full = on == 1; // 2, 3: events around the one-wave render kernel only (two per frame instead of four)
    c->timing_period = on == 3 ? 8 : 1; // 3: on every 8th frame only
    if (on) {
        c->timing_count = 0; c->timing_frame = 0;
        return ensure_timing_ring(c); // here, not in the first timed frame
    }
    return VRT_HIP_OK;
}

int vrt_hip_get_kernel_timing(vrt_hip_ctx *c, double *render_ms, double *dense_ms, double *lists_ms, uint64_t *launches)
{
    if (!c) return VRT_HIP_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = std::min<uint64_t>(c->timing_count, vrt_hip_ctx::TIMING_RING);
    double sr = 0, sd = 0, sl = 0;
    for (uint64_t i = 0; i < n; ++i) {
        hipEvent_t *e = &c->tev[4 * i];
        HIPCHK(c, hipEventSynchronize(e[c->timing_full ? 3 : 2]));
        float a = 0, b = 0, d = 0;
        HIPCHK(c, hipEventElapsedTime(&b, e[1], e[2]));
        if (c->timing_full) {
            HIPCHK(c, hipEventElapsedTime(&a, e[0], e[1]));
            HIPCHK(c, hipEventElapsedTime(&d, e[2], e[3]));
        }
        sl += a; sr += b; sd += d;
    }
    if (render_ms) *render_ms = n ? sr / n : 0.0;
    if (dense_ms) *dense_ms = n ? sd / n : 0.0;
    if (lists_ms) *lists_ms = n ? sl / n : 0.0;
    if (launches) *launches = n;
    return VRT_HIP_OK;
}

int vrt_hip_get_stats(vrt_hip_ctx *c, vrt_hip_stats *out)
{
    if (!c || !out) return VRT_HIP_ERR_INVALID;
    *out = c->last;
    return VRT_HIP_OK;
}

} // extern "C"
