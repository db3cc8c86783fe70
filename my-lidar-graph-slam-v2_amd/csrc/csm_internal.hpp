/* csm_internal.hpp -- what the translation units of libcsm_hip.so share on the host side: the
 * context (device grids, workspaces, tuning switches, graphs), error / timing helpers and the owners
 * of device and pinned memory (DevBuf, PinBuf: move-only, freed by their destructors, grown by grow()),
 * and the plumbing every unit's host side is written in: launched_ok, align256 / Carve, reserve, ScanTable,
 * take_event / CallSpan / ScopedTimer, clock_us.
 * csm_api.hip (matchers), csm_map_api.hip (map updates), csm_cost_api.hip (cost / covariance /
 * refinement) and csm_group.hip (several GPUs in one process) are compiled on their own. */
#ifndef CSM_INTERNAL_HPP
#define CSM_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <limits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <tuple>
#include <atomic>
#include <utility>
#include <vector>

#include "csm_device.hpp"
#include "csm_launch.hpp"
#include "../../include/csm_hip.h"

using namespace csm;

/* ------------------------------------------------------------------ ctx */

namespace csm_host {

/* bytes held by all live owners of the process: [0] device, [1] pinned (csm_debug_live_bytes) */
inline std::atomic<int64_t> g_live_bytes[2];

/* The owner of one hipMalloc (DevBuf) or hipHostMalloc (PinBuf) block: move-only, freed by its
 * destructor. Whoever drops a buffer that a queued kernel or copy may still read synchronises
 * first. Grown by grow() (below), never by hand. */
template <bool Pinned>
struct HipBuf {
    void*  p = nullptr;
    size_t cap = 0;

    HipBuf() = default;
    HipBuf(const HipBuf&) = delete;
    HipBuf& operator=(const HipBuf&) = delete;
    HipBuf(HipBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    HipBuf& operator=(HipBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~HipBuf() { reset(); }

    template <class T> T* as() const { return static_cast<T*>(p); }
    void reset()
    {
        if (p) {
            (void)(Pinned ? hipHostFree(p) : hipFree(p));
            g_live_bytes[Pinned] -= (int64_t)cap;
        }
        p = nullptr;
        cap = 0;
    }
    bool alloc(size_t bytes)       /* into an empty owner */
    {
        if ((Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes)) != hipSuccess) {
            p = nullptr;
            return false;
        }
        cap = bytes;
        g_live_bytes[Pinned] += (int64_t)bytes;
        return true;
    }
};
using DevBuf = HipBuf<false>;
using PinBuf = HipBuf<true>;

/* A level of a map: `cells` points into its own buffer, or (a window-1 level above level 0) at the
 * base's cells. Move-only, through `own`. */
struct Level {
    int       win = 1;
    uint16_t* cells = nullptr;   /* pitched rows*pitch */
    DevBuf    own;               /* empty for an alias of the base */
    bool      stale = false;     /* derived from a base that was rebuilt since */
    bool owned() const { return own.p != nullptr; }
};

struct DeviceGrid;

/* Phase-major copy of a box-max(L) level of a map (k_phase_map): the grid the coarse pass of the
 * two-phase search scores on. */
struct PhaseMap {
    std::unique_ptr<DeviceGrid> grid;
    int hp = 0, wp = 0, pad = 0;
    const uint16_t* built_from = nullptr;   /* the level's buffer, its shape and the base epoch it was built at */
    int from_rows = 0, from_cols = 0, from_pitch = 0;
    uint64_t epoch = 0;
};

/* "PatchSize": 16 (launcher_settings_default.json:178): the block size of maps uploaded dense */
constexpr int kDefaultLog2Block = 4;

/* Move-only (its buffers are owners): a copy does not compile. */
struct DeviceGrid {
    int rows = 0, cols = 0, pitch = 0;
    uint64_t base_epoch = 0;          /* bumped whenever level 0's cells change */
    std::map<int, PhaseMap> phase;    /* by box-max window L */
    int known_r0 = 0, known_c0 = 0;   /* first row / column holding a known cell */
    std::vector<Level> levels;   /* levels[0] is the uploaded grid */
    /* expanded, zero-padded pair-row copy of level 0 for the fine kernel's LDS-DMA
     * staging (k_expand_pairs); rebuilt when the base changes or a window needs more padding */
    DevBuf xg;                   /* uint32_t */
    int xg_pad = 0, xg_pitch = 0;
    bool xg_stale = true;
    /* the same layout holding float(499 v + 32268 (v != 0)) per cell: source of the fp32 bound
     * pass of the joint fine level (k_expand_pairs_f); follows xg */
    DevBuf xgf;                  /* float */
    bool xgf_valid = false;
    /* block-allocation bitmap for the cost function's ProbabilityOr(.., 0.5): one byte per block
     * of 2^alloc_log2 x 2^alloc_log2 cells. alloc_derived: it follows the cells (a block is
     * allocated iff it holds a known cell) and is rebuilt when alloc_stale. Otherwise it is the
     * reference's state as given (csm_set_block_allocation, csm_upload_grid_blocks) or carried
     * through the map builds, and never stale (include/csm_hip.h, csm_set_block_allocation). */
    DevBuf alloc;                /* uint8_t */
    int alloc_log2 = kDefaultLog2Block, alloc_bcols = 0;
    bool alloc_derived = true, alloc_stale = true;
};

struct TimedSpan {
    hipEvent_t a, b;
};

struct KernelTimer {
    std::vector<TimedSpan> spans;
    double  total_ms = 0.0;
    int64_t launches = 0;
};

} /* namespace csm_host */
using namespace csm_host;

/* Launch-shape switches and forced shapes. Resolved ONCE, in csm_create: the switches from
 * csm_config.tuning_off (CSM_TUNE_NO_*, A/B measurements and tests); the forced shapes only
 * in tuning builds (-DCSM_TUNING, tools/build_variant.sh), from the environment. Nothing on a
 * launch path reads the environment. */
struct Tuning {
    bool lane_map = true;      /* conflict-free thread -> candidate table (lane_map_for) */
    bool xcd_map = true;       /* a job's workgroups on one XCD (xcd_block) */
    bool pair_tail = true;     /* a window's last row block as an R = 6 launch */
    bool two_slices = true;    /* batch fine kernel takes two theta slices per workgroup */
    bool joint = true;         /* ... on joint entry lists of the two slices (k_binj / k_score_joint_batch) */
    bool bound_pass = true;    /* ... preceded by the packed-fp32 bound pass; the exact kernel skips blocks that cannot win */
    int  two_phase = 0;        /* single large windows coarse-first: 0 by size, 1 always, -1 never */
    bool graphs = true;        /* repeated single-query launch chains replayed as HIP graphs */
    bool tile_split = true;    /* small single windows: tile list split over blockIdx.z */
    bool map_host_projection = false;   /* map building: hit points on the host */
    bool greedy_literal = false;        /* hill climbing: every decision from the literal sums */
    int  theta_major = -1;     /* -1: by launch size */
    int  fine_slices = 0, force_r = 0, pair_r = 0, pair_ncbx = 0, pair_groups = 0, pair_ls = 0,
         pair_tail_ls = 0, nbuf = 0, map_unc_cap = 0;
    bool plan_debug = false, host_timing = false;
};

struct csm_ctx {
    int device = 0;
    Tuning tune;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<uint64_t, DeviceGrid> grids;
    DevBuf lut_dev;                  /* double[65536]: csm_host_probability_lut */
    /* workspaces */
    DevBuf hits, sorted, tiles, ntiles, misc, coarse_s, coarse_k, best, dump_s, dump_k, scratch;
    DevBuf b_prod, b_hits, b_sorted, b_tiles, b_ntiles, b_lvl, b_best, b_jobs, b_out, b_abest, bound_stats, b_items, tp_items, ph_hits;
    /* single-query launch chains as HIP graphs (csm_correlative_match): one per launch shape, keyed by
     * everything that is baked into the nodes; alloc_epoch changes whenever a device buffer the
     * nodes point at may have moved */
    uint64_t alloc_epoch = 0;
    bool capturing = false;
    struct RecordedChain {
        hipGraphExec_t exec = nullptr;
        csm::ScoreJob fine;          /* the fine-level job baked into the chain: last_run.fine after a replay */
    };
    std::map<std::vector<uint64_t>, RecordedChain> graphs;
    std::map<std::vector<uint64_t>, int> graph_seen;
    bool last_graph_replayed = false;            /* csm_last_search_info: the last match was a replay */
    PinBuf q_pin;                    /* [ProjJob | angles | ranges] up, [record | uncertified count] back */
    DevBuf q_dev;
    /* What the last single-window launch chain (csm_window.hip: a driver, or the replay of a recorded
     * graph) left behind, for resolve_ties and csm_last_search_info, which may run in a later call. */
    struct LastRun {
        /* the chain's fine-level job, for the tie collection pass: its flag word and two-phase
         * eligibility levels are facts of that launch, not of the window alone */
        csm::ScoreJob fine = {};
        int64_t nominal = 0, coarse_nodes = 0, fine_candidates = 0;
        /* coarse-first searches: blocks kept (= items of the work list, a device counter) of
         * blocks_total, each of block_candidates candidates */
        const uint32_t* kept_dev = nullptr;
        int64_t blocks_total = 0, block_candidates = 0;
    } last_run;
    DevBuf fine_s, fine_k, tie, ex_fine, ex_fine_k, ex_coarse, ex_coarse_k, scan_dev, unc, sorted_rc, b_sorted_rc;
    std::map<std::array<int, 4>, DevBuf> lane_maps;   /* lane_map_for(): (cbx, groups, R, LS) -> uint16_t table */
    PinBuf pin;                   /* staging of csm_upload_grid */
    PinBuf pin_scans;             /* staging of a batch's scans */
    /* cost / refinement batches: device scans + job table, host staging */
    DevBuf c_scans, c_jobs, box_jobs;
    std::vector<csm::BoxJob> box_stage;
    std::vector<double> c_stage;
    std::vector<csm::CostJob> c_job_stage;
    /* greedy-endpoint / hill-climbing batches (csm_greedy_api.hip): scans, job table + outputs,
     * rank scratch of scans too long for LDS, the cost tables */
    DevBuf g_scans, g_jobs, g_scratch, g_tab;
    /* K best poses per window (csm_peaks_api.hip): score volumes of a chunk, its scans + hit indices,
     * job table + records, pinned staging */
    DevBuf pk_vol, pk_hits, pk_tab;
    PinBuf pk_pin;
    /* volume covariance (csm_volume_api.hip) on top of the peaks' owners: job table, weight tables,
     * workgroup records + results; pinned staging */
    DevBuf vc_tab;
    PinBuf vc_pin;
    /* motion prior (csm_prior_api.hip) on top of the peaks' owners: job table, workgroup records +
     * results; pinned staging */
    DevBuf pr_tab;
    PinBuf pr_pin;
    /* likelihood-field maps (csm_likelihood_api.hip): table, job per map, counters; pinned staging */
    DevBuf lf_tab;
    PinBuf lf_pin;
    /* distance fields (csm_distance_api.hip): table, job per map, counters; the column pass's offsets of a
     * chunk of maps (and the transform's two outputs); pinned staging */
    DevBuf dt_tab, dt_work;
    PinBuf dt_pin;
    /* free-space check of loop candidates (csm_ray_api.hip): a chunk's table + scans, its work block
     * (uncertified list, records, per-beam words, ray records, patches); pinned staging up and back */
    DevBuf rc_tab, rc_work;
    PinBuf rc_pin, rc_back;
    /* pose sets (csm_poses_api.hip): a call's tables, scans and poses; its work block (marked poses, records,
     * weights, ancestors, triples, prefix sums); the host's indices of the marked poses; pinned staging */
    DevBuf ps_tab, ps_work, ps_fix;
    PinBuf ps_pin, ps_back;
    /* loop search (csm_loopsearch_api.hip): a call's node arrays and query table with its records and
     * per-query counts behind them; pinned staging, up and then back */
    DevBuf ls_dev;
    PinBuf ls_pin;
    /* appearance search (csm_appearance_api.hip): a call's upload with its ring sums and read-back block
     * behind it, the pair table of one chunk of queries; pinned staging, up and then back */
    DevBuf ap_dev, ap_table;
    PinBuf ap_pin;
    /* loop-edge consistency (csm_consistency_api.hip): a call's edge records, adjacency, per-seed cliques and
     * results; pinned staging, up and then back */
    DevBuf lc_dev;
    PinBuf lc_pin;
    /* pose-graph optimization (csm_posegraph_api.hip): graph, structure, work vectors; host staging */
    DevBuf pg_buf;
    DevBuf pg_s;                  /* the dense Schur complement of the direct solver (blocked path) */
    std::vector<uint8_t> pg_stage;
    DevBuf pg_cov;                /* csm_pose_graph_marginals: the columns of S^-1, the pair lists, the records */
    std::vector<uint8_t> pg_cov_stage;
    /* the final records of the last batch call in query order (csm_copy_last_batch_records) */
    DevBuf rec_dev;
    int rec_n = 0;
    std::vector<csm_result> rec_patch;            /* host copies of records fixed up after the device pass */
    /* map building */
    DevBuf m_rays, m_recs, m_cell, m_lists, m_cnt, m_lut;
    DevBuf m_alloc;                               /* the old map's allocation bitmap during a build */
    double m_lut_hit = -1.0, m_lut_miss = -1.0;   /* probabilities the update tables were built for */
    int m_cus = 0;                                /* compute units of the device (the batch's persistent kernel) */
    DevBuf m_btab;                                /* csm_construct_maps_from_scans: job and prefix tables */
    std::vector<double> stage;                    /* host staging of one scan (angles, ranges) */
    /* pinned job-table blocks of csm_score_windows_dev calls (sources of asynchronous
     * uploads), each kept until the event recorded behind its launch chain has fired; an entry
     * taken out must move its block back to pin_free (dropping it frees the block) */
    std::vector<std::pair<hipEvent_t, PinBuf>> resident_hold;
    unsigned flag_toggle = 0;     /* two flag words, used alternately: k_finalize of query i
                                     clears the word of query i + 1 */
    bool flags_ready = false;
    bool fine_acc_dirty = false;  /* a tile-split launch was issued but its arg-max pass (which
                                     clears the accumulators) was not: clear before reuse */
    int timing = 0;               /* 0 off, 1 every kernel, 2 the fine scoring kernel only */
    std::map<std::string, KernelTimer> timers;
    std::vector<hipEvent_t> event_pool;
    /* pinned staging blocks of the batch entries' job tables, reused once the copy
     * that reads them has run (first fit) */
    std::vector<PinBuf> pin_free;
};

namespace csm_host {


inline int fail(csm_ctx* ctx, int code, const char* fmt, ...)
{
    if (ctx) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        ctx->err = buf;
    }
    return code;
}

#define HIP_TRY(ctx, expr)                                                        \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess)                                                     \
            return fail(ctx, CSM_EIO, "%s failed: %s (%s:%d)", #expr,             \
                        hipGetErrorString(e_), __FILE__, __LINE__);               \
    } while (0)

/* The one way an owner grows: when `bytes` exceed b's capacity, free it (after the stream has
 * drained, if it held a buffer) and allocate `want` >= bytes, the site's growth policy; the old
 * contents are not kept. `moves_graph_inputs`: recorded graphs may point at b (alloc_epoch). */
template <bool Pinned>
int grow(csm_ctx* ctx, HipBuf<Pinned>& b, size_t bytes, size_t want, bool moves_graph_inputs)
{
    if (bytes <= b.cap)
        return CSM_OK;
    if (moves_graph_inputs)
        ++ctx->alloc_epoch;
    if (b.p)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    b.reset();
    if (!b.alloc(want))
        return fail(ctx, CSM_ENOMEM, "%s(%zu) failed", Pinned ? "hipHostMalloc" : "hipMalloc", want);
    return CSM_OK;
}

/* a workspace of the context: 25 % + 256 bytes of slack; never grows during graph capture */
inline int ensure(csm_ctx* ctx, DevBuf& b, size_t bytes)
{
    if (bytes > b.cap && ctx->capturing)
        return fail(ctx, CSM_EIO, "internal: a workspace would grow during graph capture");
    return grow(ctx, b, bytes, bytes + bytes / 4 + 256, true);
}

/* a workspace no recorded graph points at: the same slack, pinned or device */
template <bool Pinned>
int reserve(csm_ctx* ctx, HipBuf<Pinned>& b, size_t n) { return grow(ctx, b, n, n + n / 4 + 256, false); }

using csm_launch::keep_first;       /* what the units with kernels of their own launch through */
using csm_launch::launch;
using csm_launch::launch_lds;

/* What every wrapper of the launch layer (csm_launch.hpp) returns: a HIP error code, or -1 for "no kernel
 * instantiated". */
inline int launched_ok(csm_ctx* ctx, int e, const char* what)
{
    if (e < 0)
        return fail(ctx, CSM_EINVAL, "internal: no %s kernel for this launch shape", what);
    if (e != 0)
        return fail(ctx, CSM_EIO, "%s kernel launch failed: %s", what, hipGetErrorString((hipError_t)e));
    return CSM_OK;
}

constexpr size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

/* one allocation carved into 256-byte aligned pieces: take() returns a piece's offset, `off` is the size so far */
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        const size_t o = off;
        off += align256(bytes);
        return o;
    }
};

/* The distinct scans of a call in first-use order. A scan is its two arrays and its length: the same arrays
 * at another length are another scan. */
struct ScanTable {
    std::map<std::tuple<const double*, const double*, int>, long long> seen;
    std::vector<int> first_use;   /* the users that fed a scan the table did not hold: they copy it */
    long long beams = 0;          /* of the distinct scans */

    /* the slot of `user`'s scan, counted in beams */
    long long slot(const csm_scan& sc, int user)
    {
        const auto ins = seen.emplace(std::make_tuple(sc.angles, sc.ranges, (int)sc.n_points), beams);
        if (ins.second) {
            first_use.push_back(user);
            beams += sc.n_points;
        }
        return ins.first->second;
    }
};

/* Microseconds on the clock of the timing fields. */
inline double clock_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* an event of the context's pool, or a new one; null: none could be created */
inline hipEvent_t take_event(csm_ctx* ctx)
{
    hipEvent_t e = nullptr;
    if (!ctx->event_pool.empty()) {
        e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
    } else {
        (void)hipEventCreate(&e);
    }
    return e;
}

/* The events of one call's device_us (none for a caller who does not want it): back into the context's pool
 * however the call ends. */
struct CallSpan {
    csm_ctx* ctx;
    hipEvent_t a, b;
    explicit CallSpan(csm_ctx* c, bool wanted = true)
        : ctx(c), a(wanted ? take_event(c) : nullptr), b(wanted ? take_event(c) : nullptr) {}
    CallSpan(const CallSpan&) = delete;
    CallSpan& operator=(const CallSpan&) = delete;
    ~CallSpan()
    {
        if (a) ctx->event_pool.push_back(a);
        if (b) ctx->event_pool.push_back(b);
    }
};

struct ScopedTimer {
    csm_ctx* ctx;
    hipEvent_t a = nullptr, b = nullptr;
    const char* name;
    ScopedTimer(csm_ctx* c, const char* n) : ctx(c), name(n)
    {
        if (!ctx->timing || ctx->capturing ||
            (ctx->timing == 2 && std::strcmp(n, "score_fine") != 0 && std::strcmp(n, "score_bound") != 0))
            return;
        a = take_event(ctx);
        b = take_event(ctx);
        (void)hipEventRecord(a, ctx->stream);
    }
    ~ScopedTimer()
    {
        if (!a)
            return;
        (void)hipEventRecord(b, ctx->stream);
        ctx->timers[name].spans.push_back({ a, b });
    }
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

/* A "no return" beam (inf / NaN range) has no hit point; the reference's scan
 * filters drop such beams before a matcher sees the scan. The library refuses
 * them instead of converting a non-finite coordinate to an int. */
inline bool scan_is_finite(const csm_scan* scan)
{
    for (int i = 0; i < scan->n_points; ++i)
        if (!std::isfinite(scan->ranges[i]) || !std::isfinite(scan->angles[i]))
            return false;
    return std::isfinite(scan->relative_sensor_pose[0]) && std::isfinite(scan->relative_sensor_pose[1]) &&
           std::isfinite(scan->relative_sensor_pose[2]);
}

/* A map frame the projections can divide by: a finite resolution above zero, finite offsets. */
inline bool geometry_is_finite(const csm_geometry* geom)
{
    return std::isfinite(geom->resolution) && geom->resolution > 0.0 && std::isfinite(geom->offset_x) &&
           std::isfinite(geom->offset_y);
}

inline DeviceGrid* find_grid(csm_ctx* ctx, uint64_t id)
{
    auto it = ctx->grids.find(id);
    return it == ctx->grids.end() ? nullptr : &it->second;
}

/* defined in csm_api.hip */
/* drops g's levels above the base (keep_base) or all its memory; the scalars that steer the next
 * build (xg_pad) stay. The caller has synchronised the stream. */
void free_levels(DeviceGrid& g, bool keep_base);
/* map_id's grid taken out of the context with its memory released (the caller has synchronised):
 * a rebuild starts from it and is registered again only once it has succeeded */
DeviceGrid take_grid(csm_ctx* ctx, uint64_t map_id);
/* level 0's cells changed: drop the phase-major copies and bump base_epoch (the caller has
 * synchronised the stream that may still read them) */
void base_changed(DeviceGrid& g);
/* What the builders of fields from resident maps share (likelihood fields, distance fields): src_ids[i] ->
 * dst_ids[i], every field with the rows, cols and pitch of its source.
 * field_ids_ok: CSM_ENOENT for a source that is not resident, CSM_EINVAL for a destination that appears
 * twice or is one of the sources (`what` names the field in the message).
 * alloc_field_bases: the new base levels, owned by the caller until every one of them is built.
 * register_fields: the caller has built bases[i] and synchronised the stream; known[2 i], known[2 i + 1] are
 * the first known row / column of its cells. dst_ids[i] is left in the state csm_upload_grid of those cells
 * leaves it in: an old map under the id has its memory released and its copies dropped, base_epoch bumped. */
int field_ids_ok(csm_ctx* ctx, const char* what, const uint64_t* src_ids, const uint64_t* dst_ids, int n);
int alloc_field_bases(csm_ctx* ctx, const uint64_t* src_ids, int n, std::vector<Level>& bases);
void register_fields(csm_ctx* ctx, const uint64_t* src_ids, const uint64_t* dst_ids, int n, std::vector<Level>& bases,
                     const int32_t* known);

/* defined in csm_cost_api.hip */
/* g.alloc made current: a derived bitmap that is stale is rebuilt from the cells */
int ensure_allocation(csm_ctx* ctx, DeviceGrid& g);
/* g.alloc after a map build (g's rows, cols and cells are the new map's), on blocks of 2^log2b:
 * block (br, bc) is allocated iff block (br + carried_br0, bc + carried_bc0) of `carried`
 * (carried_brows x carried_bcols, null = nothing) is, or it holds a known cell. Queued on
 * ctx->stream; `carried` must stay alive until the stream has drained. */
int build_allocation(csm_ctx* ctx, DeviceGrid& g, int log2b, const uint8_t* carried, int carried_brows,
                     int carried_bcols, int carried_br0, int carried_bc0);

/* defined in csm_map_api.hip */
constexpr uint32_t kMapUncCap = 4096;    /* beams listed for exact recomputation per map build */
/* ctx->m_lut = the value -> value tables of one hit / one miss update for prm's probabilities */
int map_ensure_tables(csm_ctx* ctx, const csm_map_builder_params* prm);

} /* namespace csm_host */
using namespace csm_host;

#endif
