// lm_subseq.hip — subject subsequences and flanks from the resident 2-bit genomes: lm_index_subseqs, lm_index_subseq_rows,
// lm_index_genome_seqs, lm_format_subseqs (include/lexicmap_hip.h).  What `lexicmap utils subseq` and
// `lexicmap utils genome-seqs` do one region at a time from disk (seek, read, unpack), as one batched device pass.
//
//   plan      (host, lm_subseq_plan.h) per region: the record, the contig, the flanks and the clamps -> `len` bases from
//             position `start` of a record, forward or reverse complement; the regions laid out back to back in the blob,
//             each from a multiple of 16 bytes: goff = the scan of their 16-base groups.
//   k_subseq_extract   flat over the OUTPUT: a lane owns one group of 16 bases = one 16-byte store (1 KB per wavefront
//             instruction).  It finds its region by binary search in goff between the brackets its workgroup's tile has
//             (as k_pair_emit does), loads the one or two aligned 32-bit words that hold its 16 bases at any of the four
//             2-bit phases, and writes "ACGT"[code] - for the '-' strand walking the source downwards with 3 - code.  The
//             last group of a region is zero-filled behind its last base.  A lane dereferences only bytes that hold bases
//             of its own region: where an aligned word reaches over the region's first or last byte it is put together
//             from single byte loads.
//   pieces    the blob passes through two device buffers cut from the scratch arena: while piece p is copied to the
//             result's pinned host blob on the second lane's stream, piece p + 1 is extracted on the first lane's.
// A host-resident genome is read where it lives, through the same aligned loads (a wavefront covers one contiguous run of
// 256 - 260 bytes): no staging pass.
// Memory: 24 B per region of tables (16 B region + 8 B scan) and two piece buffers on the device; the blob in pinned host memory.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "lm_internal.h"
#include "lm_seed_walk.h"
#include "lm_subseq_plan.h"

namespace lm {

// `len` bases from base `start` of the 2-bit genome at src (device store or pinned host memory); top bit of len_rc: '-' strand.
// The plan refuses a region that does not fit these fields (LM_SS_MAX_START, LM_SS_MAX_LEN in lm_subseq_plan.h).
struct SsDevRegion {
    const uint8_t *src;
    uint32_t start, len_rc;
};
struct SsKernArgs {
    const SsDevRegion *reg;
    const int64_t *goff; // [regions + 1] first group of every region
    int64_t r0, r1;      // the regions that own a group of this piece
    int64_t g0, n;       // the piece: groups [g0, g0 + n)
    uint8_t *out;        // n * 16 bytes
};

typedef uint32_t ss_u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_subseq_extract(SsKernArgs a) {
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < a.n; t0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t1 = (t0 + (int64_t)blockDim.x < a.n ? t0 + (int64_t)blockDim.x : a.n) - 1;
        int64_t rf, rl;
        sw_tile_lists(a.goff, a.r0, a.r1, a.g0 + t0, a.g0 + t1, &rf, &rl);
        const int64_t t = t0 + threadIdx.x;
        if (t > t1) continue;
        const int64_t G = a.g0 + t;
        const int64_t r = sw_last_le(a.goff, rf, rl, G); // the last region that starts at or before G: it has groups, G is one of them
        const SsDevRegion R = a.reg[r];
        const int64_t len = (int64_t)(R.len_rc & 0x7fffffffu), start = R.start;
        const bool rc = (R.len_rc >> 31) != 0;
        const int64_t o0 = (G - a.goff[r]) * LM_SS_GROUP;                           // the group's first output base
        uint32_t w[4];
        ss_group(R.src, start, len, rc, o0, w); // (lm_subseq_plan.h: the host runs the same lane)
        const ss_u32x4 o = {w[0], w[1], w[2], w[3]};
        __builtin_nontemporal_store(o, (ss_u32x4 *)(a.out + t * LM_SS_GROUP)); // written once, read by the copy engine
    }
}

// (not the pipeline's parallel_for: the thread cap and the chunking differ, and with them the host's timing)
template <typename F> static void ss_parallel_for(int64_t n, int64_t grain, F f) {
    if (n <= 0) return;
    const int nt = (int)std::min<int64_t>((n + grain - 1) / grain, std::min(16u, std::max(1u, std::thread::hardware_concurrency())));
    if (nt <= 1) {
        f((int64_t)0, n);
        return;
    }
    const int64_t per = (n + nt - 1) / nt;
    std::exception_ptr err;
    std::mutex emu;
    auto body = [&](int64_t a, int64_t b) {
        try {
            f(a, b);
        } catch (...) {
            std::lock_guard<std::mutex> l(emu);
            if (!err) err = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < nt; i++)
        if (i * per < n) th.emplace_back(body, i * per, std::min(n, (i + 1) * per));
    body((int64_t)0, std::min(n, per));
    for (auto &t : th) t.join();
    if (err) std::rethrow_exception(err);
}

static SsRecView ss_view(const HostGenome &G) {
    SsRecView v;
    v.seq_sizes = G.seq_sizes.data();
    v.seq_ids = G.seq_ids.data();
    v.nseqs = (int32_t)std::min(G.seq_sizes.size(), G.seq_ids.size());
    v.len = G.len;
    v.key = G.bg;
    return v;
}

// the local records of every genome id asked for, in chunk order (a sharded handle sees its own genomes)
typedef std::unordered_map<std::string, std::vector<int32_t>> SsNames;
static void ss_collect_names(const lm_index *ix, SsNames &names) {
    if (names.empty()) return;
    const HostIndex &h = ix->host;
    for (size_t l = 0; l < h.genomes.size(); l++) {
        auto it = names.find(h.genomes[l].id);
        if (it != names.end()) it->second.push_back((int32_t)l);
    }
    auto chunk = [&](int32_t l) {
        auto c = h.chunk_of.find(h.genomes[(size_t)l].bg);
        return c == h.chunk_of.end() ? 0 : c->second.idx;
    };
    for (auto &kv : names)
        std::stable_sort(kv.second.begin(), kv.second.end(), [&](int32_t x, int32_t y) { return chunk(x) < chunk(y); });
}

// the handle as the plan sees it (lm_subseq_plan.h)
struct SsIndexLookup : SsLookup {
    const lm_index *ix;
    SsNames names;
    explicit SsIndexLookup(const lm_index *ix_) : ix(ix_) {}
    int32_t local_of(uint64_t key) const override {
        const auto f = ix->bg2local.find(key);
        return f == ix->bg2local.end() ? -1 : f->second;
    }
    // a sharded handle knows the records of the other shards by their tables; a synthetic one by their number
    bool elsewhere(uint64_t key) const override {
        const HostIndex &h = ix->host;
        if (h.shard_count <= 1) return false;
        if (!h.synthetic) return h.other_of.count(key) != 0;
        const uint64_t index = key & 0x1ffff, batch = key >> 17;
        return index < 5000 && batch <= (uint64_t)h.synth_genomes / 5000 && (int64_t)(batch * 5000 + index) < h.synth_genomes;
    }
    const std::vector<int32_t> *records_of(const char *genome_id) const override {
        const auto f = names.find(genome_id);
        return f == names.end() ? nullptr : &f->second;
    }
    SsRecView record(int32_t local) const override { return ss_view(ix->host.genomes[(size_t)local]); }
};
static_assert(LM_SS_BY_NAME == LM_REGION_BY_NAME && SS_NOT_LOCAL == LM_SUBSEQ_NOT_LOCAL && SS_OK == LM_SUBSEQ_OK, "lm_subseq_plan.h mirrors the public header");

} // namespace lm

struct lm_subseqs {
    std::vector<lm_subseq_info> info;
    char *blob = nullptr; // pinned
    lm_subseq_stats stats;
    bool genome_seqs = false;
    ~lm_subseqs() {
        if (blob) (void)hipHostFree(blob);
    }
};

namespace lm {

// the two piece buffers, their events and the copy stream of one call; whatever happens, nothing is released while the
// device may still use it
struct SsPipe {
    lm_index *ix;
    hipStream_t sx, sy;
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t start[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    SsPipe(lm_index *ix_, hipStream_t x, hipStream_t y) : ix(ix_), sx(x), sy(y) {}
    ~SsPipe() {
        (void)hipStreamSynchronize(sx);
        (void)hipStreamSynchronize(sy);
        for (int b = 0; b < 2; b++) {
            if (buf[b]) (void)ix->lane[0].arena.release(buf[b]);
            for (hipEvent_t e : {start[b], done[b], copied[b]})
                if (e) (void)hipEventDestroy(e);
        }
    }
};

// regions [0, n) through get(i) -> the result
template <typename Get> static void subseq_run(lm_index *ix, const char *who, size_t n, Get get, const lm_subseq_opt &opt, lm_subseqs &res) {
    const double t_begin = now_ms();
    const HostIndex &h = ix->host;
    // ---- plan (lm_subseq_plan.h: the rule, the statuses, the refusals)
    SsIndexLookup look(ix);
    for (size_t i = 0; i < n; i++) {
        const lm_region rg = get(i);
        if (rg.key == LM_REGION_BY_NAME && rg.genome_id) look.names.emplace(rg.genome_id, std::vector<int32_t>());
    }
    ss_collect_names(ix, look.names);
    auto region = [&](size_t i) {
        const lm_region rg = get(i);
        SsRegion r;
        r.key = rg.key;
        r.genome_id = rg.genome_id;
        r.seq_id = rg.seq_id;
        r.seq_idx = rg.seq_idx;
        r.rc = rg.rc;
        r.begin = rg.begin;
        r.end = rg.end;
        return r;
    };
    std::vector<SsItem> items;
    std::string refusal;
    if (!ss_plan(look, h.contig_interval, who, n, region, opt.upstream, opt.downstream, opt.ignore_errors != 0, items, refusal,
                 [](int64_t m, auto f) { ss_parallel_for(m, 1 << 16, f); }))
        throw ArgError(refusal);
    std::vector<int64_t> lens(n), goff(n + 1);
    for (size_t i = 0; i < n; i++) lens[i] = items[i].status == SS_OK ? items[i].w.len : 0;
    const int64_t groups = ss_layout(lens.data(), n, goff.data());
    const size_t blob_bytes = (size_t)groups * LM_SS_GROUP;
    // ---- the result's tables
    res.info.resize(n);
    int64_t answered = 0, bases = 0;
    for (size_t i = 0; i < n; i++) {
        const SsItem &it = items[i];
        lm_subseq_info &o = res.info[i];
        memset(&o, 0, sizeof o);
        o.key = it.key;
        o.seq_idx = it.seq_idx;
        o.status = it.status;
        o.rc = it.rc;
        o.begin = it.w.begin;
        o.end = it.w.end;
        o.off = goff[i] * LM_SS_GROUP;
        o.len = lens[i];
        if (it.local >= 0) {
            const HostGenome &G = h.genomes[(size_t)it.local];
            o.genome_id = G.id.c_str();
            if (it.seq_idx >= 0 && it.seq_idx < (int32_t)G.seq_ids.size()) o.seq_id = G.seq_ids[(size_t)it.seq_idx].c_str();
        }
        if (it.status == SS_OK) {
            answered++;
            bases += lens[i];
        }
    }
    const double t_alloc = now_ms();
    if (hipHostMalloc((void **)&res.blob, std::max<size_t>(blob_bytes, LM_SS_GROUP), hipHostMallocDefault) != hipSuccess) {
        res.blob = nullptr;
        (void)hipGetLastError();
        throw DeviceOOM(std::string(who) + ": the host could not pin the " + std::to_string(blob_bytes >> 20) + " MB of the base blob");
    }
    res.stats.regions = (int64_t)n;
    res.stats.answered = answered;
    res.stats.bases = bases;
    res.stats.blob_bytes = (int64_t)blob_bytes;
    const double t_plan = now_ms();
    res.stats.ms_plan = t_alloc - t_begin;
    res.stats.ms_alloc = t_plan - t_alloc;
    if (groups > 0) {
        // ---- device tables
        std::vector<SsDevRegion> reg(n);
        for (size_t i = 0; i < n; i++) {
            const SsItem &it = items[i];
            SsDevRegion &d = reg[i];
            d.src = nullptr;
            d.start = 0;
            d.len_rc = 0;
            if (lens[i] == 0) continue;
            // (a host-resident genome is read where it lives: lm_kernels.hip, k_stage_genome_bits, lists the kernels that may)
            d.src = !ix->g_hptr.empty() && ix->g_hptr[(size_t)it.local] ? ix->g_hptr[(size_t)it.local] : ix->d_gbits.p + h.genomes[(size_t)it.local].bits_off;
            d.start = (uint32_t)it.w.src;
            d.len_rc = (uint32_t)lens[i] | (it.rc ? 0x80000000u : 0u);
        }
        const hipStream_t sx = ix->lane[0].main.st;
        if (!ix->lane[1].main.st) HIPCHK(hipStreamCreate(&ix->lane[1].main.st));
        const hipStream_t sy = ix->lane[1].main.st;
        DBuf<SsDevRegion> d_reg;
        DBuf<int64_t> d_goff;
        d_reg.alloc_exact(n);
        d_goff.alloc_exact(n + 1);
        HIPCHK(hipMemcpyAsync(d_reg.p, reg.data(), n * sizeof(SsDevRegion), hipMemcpyHostToDevice, sx));
        HIPCHK(hipMemcpyAsync(d_goff.p, goff.data(), (n + 1) * 8, hipMemcpyHostToDevice, sx));
        // ---- pieces: two buffers from the scratch arena; the budget halves until the arena can give them
        const char *env = getenv("LM_SUBSEQ_PIECE_BYTES");
        int64_t piece = env ? std::max<int64_t>(LM_SS_GROUP, atoll(env) / LM_SS_GROUP * LM_SS_GROUP) : (int64_t)256 << 20;
        piece = std::min<int64_t>(piece, (int64_t)blob_bytes);
        SsPipe pp(ix, sx, sy);
        while (true) {
            const int nbuf = piece < (int64_t)blob_bytes ? 2 : 1;
            try {
                for (int b = 0; b < nbuf; b++) pp.buf[b] = ix->lane[0].arena.alloc((size_t)piece);
                break;
            } catch (const DeviceOOM &e) {
                (void)hipGetLastError();
                for (int b = 0; b < 2; b++)
                    if (pp.buf[b]) {
                        (void)ix->lane[0].arena.release(pp.buf[b]);
                        pp.buf[b] = nullptr;
                    }
                if (env || piece <= ((int64_t)1 << 20))
                    throw DeviceOOM(std::string(who) + ": two piece buffers of " + std::to_string(piece >> 20) + " MB do not fit the device beside the index: " + e.what());
                piece = (piece / 2 + LM_SS_GROUP - 1) / LM_SS_GROUP * LM_SS_GROUP;
            }
        }
        std::vector<SsPiece> pieces;
        ss_pieces(goff.data(), n, piece, pieces);
        for (int b = 0; b < 2; b++) {
            HIPCHK(hipEventCreate(&pp.start[b]));
            HIPCHK(hipEventCreate(&pp.done[b]));
            HIPCHK(hipEventCreateWithFlags(&pp.copied[b], hipEventDisableTiming));
        }
        double ms_dev = 0;
        auto retire = [&](int b) { // the piece that used buffer b is in the blob
            HIPCHK(hipEventSynchronize(pp.copied[b]));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, pp.start[b], pp.done[b]));
            ms_dev += ms;
        };
        for (size_t p = 0; p < pieces.size(); p++) {
            const SsPiece &P = pieces[p];
            const int b = pp.buf[1] ? (int)(p & 1) : 0;
            if (p >= (pp.buf[1] ? 2u : 1u)) retire(b);
            const int64_t ng = P.g1 - P.g0;
            if (ng <= 0 || (size_t)ng * LM_SS_GROUP > (size_t)piece || P.r1 <= P.r0) throw HipError(std::string(who) + ": a piece does not fit its plan");
            const SsKernArgs ka{d_reg.p, d_goff.p, P.r0, P.r1, P.g0, ng, (uint8_t *)pp.buf[b]};
            const unsigned grid = (unsigned)std::min<int64_t>((ng + 255) / 256, 1 << 16);
            HIPCHK(hipEventRecord(pp.start[b], sx));
            hipLaunchKernelGGL(k_subseq_extract, dim3(grid), dim3(256), 0, sx, ka);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(pp.done[b], sx));
            HIPCHK(hipStreamWaitEvent(sy, pp.done[b], 0));
            HIPCHK(hipMemcpyAsync(res.blob + P.g0 * LM_SS_GROUP, pp.buf[b], (size_t)ng * LM_SS_GROUP, hipMemcpyDeviceToHost, sy));
            HIPCHK(hipEventRecord(pp.copied[b], sy));
        }
        const size_t np = pieces.size(), inflight = std::min<size_t>(np, pp.buf[1] ? 2 : 1);
        for (size_t p = np - inflight; p < np; p++) retire(pp.buf[1] ? (int)(p & 1) : 0);
        HIPCHK(hipStreamSynchronize(sx)); // (the tables go out of scope)
        res.stats.pieces = (int64_t)np;
        res.stats.ms_device = ms_dev;
    }
    res.stats.ms_total = now_ms() - t_begin;
    if (getenv("LM_DEBUG"))
        fprintf(stderr, "[lm] subseq: %zu regions, %lld answered, %lld bases, %lld pieces, plan %.2f ms, pinning %.2f ms, kernels %.2f ms, total %.2f ms\n", n,
                (long long)answered, (long long)bases, (long long)res.stats.pieces, res.stats.ms_plan, res.stats.ms_alloc, res.stats.ms_device, res.stats.ms_total);
}

template <typename Get> static lm_status subseq_call(lm_index *ix, const char *who, size_t n, Get get, const lm_subseq_opt *opt_in, bool genome_seqs,
                                                     lm_subseqs **out) {
    lm_subseq_opt opt;
    lm_subseq_opt_default(&opt);
    if (opt_in) opt = *opt_in;
    std::unique_ptr<lm_subseqs> res(new lm_subseqs());
    memset(&res->stats, 0, sizeof res->stats);
    res->genome_seqs = genome_seqs;
    const lm_status rc = guarded(ix, who, ": the host could not hold the plan of the regions", [&]() { subseq_run(ix, who, n, get, opt, *res); });
    if (rc == LM_OK) *out = res.release();
    return rc;
}

} // namespace lm

extern "C" void lm_subseq_opt_default(lm_subseq_opt *o) {
    if (o) memset(o, 0, sizeof *o);
}

extern "C" lm_status lm_index_subseqs(lm_index *ix, const lm_region *regions, size_t n, const lm_subseq_opt *opt, lm_subseqs **out) {
    if (!ix || !out) return LM_ERR_ARG;
    *out = nullptr;
    if (!regions && n > 0) {
        ix->err = "lm_index_subseqs: regions is NULL but n is not 0";
        return LM_ERR_ARG;
    }
    return lm::subseq_call(ix, "lm_index_subseqs", n, [regions](size_t i) { return regions[i]; }, opt, false, out);
}

extern "C" lm_status lm_index_subseq_rows(lm_index *ix, const lm_hsp *rows, size_t n, const lm_subseq_opt *opt, lm_subseqs **out) {
    if (!ix || !out) return LM_ERR_ARG;
    *out = nullptr;
    if (!rows && n > 0) {
        ix->err = "lm_index_subseq_rows: rows is NULL but n is not 0";
        return LM_ERR_ARG;
    }
    auto get = [rows](size_t i) {
        lm_region r;
        r.key = rows[i].batch_genome;
        r.genome_id = r.seq_id = nullptr;
        r.seq_idx = rows[i].seq_idx < 0 ? INT32_MAX : rows[i].seq_idx; // (a row always names a contig: never concatenated coordinates)
        r.rc = rows[i].rc;
        r.begin = (int64_t)rows[i].tbegin + 1;
        r.end = (int64_t)rows[i].tend + 1;
        return r;
    };
    return lm::subseq_call(ix, "lm_index_subseq_rows", n, get, opt, false, out);
}

extern "C" lm_status lm_index_genome_seqs(lm_index *ix, const char *genome_id, lm_subseqs **out) {
    using namespace lm;
    if (!ix || !out) return LM_ERR_ARG;
    *out = nullptr;
    if (!genome_id) {
        ix->err = "lm_index_genome_seqs: genome_id is NULL";
        return LM_ERR_ARG;
    }
    std::vector<lm_region> regions;
    {
        std::lock_guard<std::mutex> lock(ix->mu);
        SsNames names;
        names.emplace(genome_id, std::vector<int32_t>());
        ss_collect_names(ix, names);
        const std::vector<int32_t> &recs = names.begin()->second;
        if (recs.empty()) {
            ix->err = std::string("lm_index_genome_seqs: reference name not found: ") + genome_id;
            return LM_ERR_ARG;
        }
        for (int32_t l : recs) {
            const HostGenome &G = ix->host.genomes[(size_t)l];
            for (size_t c = 0; c < G.seq_sizes.size(); c++) {
                lm_region r;
                r.key = G.bg;
                r.genome_id = r.seq_id = nullptr;
                r.seq_idx = (int32_t)c;
                r.rc = 0;
                r.begin = 1;
                r.end = std::max<int64_t>(1, G.seq_sizes[c]);
                regions.push_back(r);
            }
        }
    }
    const lm_region *rp = regions.data();
    return subseq_call(ix, "lm_index_genome_seqs", regions.size(), [rp](size_t i) { return rp[i]; }, nullptr, true, out);
}

extern "C" size_t lm_subseqs_get(const lm_subseqs *s, const lm_subseq_info **info, const char **bases) {
    if (!s) return 0;
    if (info) *info = s->info.data();
    if (bases) *bases = s->blob;
    return s->info.size();
}
extern "C" void lm_subseqs_get_stats(const lm_subseqs *s, lm_subseq_stats *stats) {
    if (s && stats) *stats = s->stats;
}
extern "C" void lm_subseqs_free(lm_subseqs *s) { delete s; }

extern "C" lm_status lm_format_subseqs(const lm_subseqs *s, const lm_hsp *rows, const char *const *query_ids, const uint32_t *query_lens, size_t nq,
                                       int line_width, char **text, size_t *len) {
    using namespace lm;
    if (!s || !text || !len) return LM_ERR_ARG;
    *text = nullptr;
    *len = 0;
    const size_t n = s->info.size();
    if (rows) {
        if (n > 0 && (!query_ids || !query_lens)) return LM_ERR_ARG;
        for (size_t i = 0; i < n; i++)
            if (rows[i].query >= nq) return LM_ERR_ARG;
    }
    const int64_t grain = 2048, nparts = ((int64_t)n + grain - 1) / grain;
    std::vector<std::string> parts((size_t)nparts);
    try {
        ss_parallel_for(nparts, 1, [&](int64_t p0, int64_t p1) {
            std::vector<char> line((size_t)1 << 12);
            for (int64_t p = p0; p < p1; p++) {
                std::string &out = parts[(size_t)p];
                for (size_t i = (size_t)(p * grain); i < std::min(n, (size_t)((p + 1) * grain)); i++) {
                    const lm_subseq_info &o = s->info[i];
                    if (o.status != LM_SUBSEQ_OK) continue; // subseq.go:233-243
                    if (s->genome_seqs) {
                        out.push_back('>');
                        out.append(o.seq_id ? o.seq_id : "");
                    } else {
                        const char *row = nullptr;
                        if (rows) {
                            const uint32_t q = rows[i].query;
                            lm_hsp r = rows[i];
                            if (!r.genome_id) r.genome_id = o.genome_id; // (rows that came from another process without names)
                            if (!r.seq_id) r.seq_id = o.seq_id;
                            int need = lm_format_row_ex(&r, query_ids[q] ? query_ids[q] : "", query_lens[q], 0, line.data(), line.size());
                            if (need >= (int)line.size()) {
                                line.resize((size_t)need + 1);
                                lm_format_row_ex(&r, query_ids[q] ? query_ids[q] : "", query_lens[q], 0, line.data(), line.size());
                            }
                            row = line.data();
                        }
                        ss_header(out, o.seq_idx >= 0 ? o.seq_id : o.genome_id, o.begin, o.end, o.rc != 0, row);
                    }
                    out.push_back('\n');
                    ss_wrap(out, s->blob + o.off, o.len, line_width);
                    out.push_back('\n');
                }
            }
        });
        std::vector<size_t> off((size_t)nparts + 1, 0);
        for (int64_t p = 0; p < nparts; p++) off[(size_t)p + 1] = off[(size_t)p] + parts[(size_t)p].size();
        char *buf = (char *)malloc(off[(size_t)nparts] + 1);
        if (!buf) return LM_ERR_NOMEM;
        ss_parallel_for(nparts, 1, [&](int64_t p0, int64_t p1) {
            for (int64_t p = p0; p < p1; p++) memcpy(buf + off[(size_t)p], parts[(size_t)p].data(), parts[(size_t)p].size());
        });
        buf[off[(size_t)nparts]] = 0;
        *text = buf;
        *len = off[(size_t)nparts];
    } catch (const std::exception &) {
        return LM_ERR_NOMEM;
    }
    return LM_OK;
}
