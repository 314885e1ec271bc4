// lm_comm.cpp - the ONE collective of the sharded search behind the C-ABI (include/lexicmap_hip.h):
// a gatherv of lm_hsp row records over RCCL (xGMI inside a node).  Every rank searched the same query batch against its
// genome shard; the merging rank needs every shard's rows, the others need nothing back - so the collective is: one
// all-gather of the counts (24 bytes per rank: rows, string bytes, flags | status), then ONE group of point-to-point transfers (ncclSend on the ranks,
// ncclRecv x (N-1) on the root: (N-1) payloads over the root's xGMI links, nothing to the ranks that do not merge).  What
// it merges into: lm_merge_sharded = the order of lib-index-search.go:2919-2921 / merge-search-results.go:142-194.
//
// RCCL is bound at run time (dlopen of librccl.so.1): a host process that already carries an RCCL (a PyTorch process
// carries its own copy) keeps using that ONE instance, and a single-GPU user of the library needs no RCCL at all.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lexicmap_hip.h"
#include "lm_merge.h"

// The few RCCL types and constants this file needs, declared here (values of rccl.h / nccl.h, stable since NCCL 2.0): the
// library is bound with dlopen, so the single-GPU build must not need the RCCL headers either.  lm_comm_* check ncclGetVersion
// after binding (point-to-point transfers exist since 2.7).
typedef struct ncclComm *ncclComm_t;
typedef struct {
    char internal[128];
} ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclUint8 = 1, ncclUint64 = 5 } ncclDataType_t;

extern thread_local std::string g_open_error; // text of the last failure without a handle (lm_last_error(NULL))

namespace {
struct Rccl {
    void *so = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int *) = nullptr;
    int version = 0;
    std::string err;
    bool ok = false;
};
Rccl &rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *names[] = {getenv("LM_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names) {
            if (!n || !*n) continue;
            r.so = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (r.so) break;
        }
        if (!r.so) {
            r.err = std::string("RCCL not found (librccl.so.1): ") + (dlerror() ? dlerror() : "");
            return;
        }
#define LM_SYM(field, name)                                                      \
    r.field = (decltype(r.field))dlsym(r.so, name);                              \
    if (!r.field) {                                                              \
        r.err = std::string("RCCL symbol missing: ") + name;                     \
        return;                                                                  \
    }
        LM_SYM(GetUniqueId, "ncclGetUniqueId")
        LM_SYM(CommInitRank, "ncclCommInitRank")
        LM_SYM(CommDestroy, "ncclCommDestroy")
        LM_SYM(AllGather, "ncclAllGather")
        LM_SYM(Send, "ncclSend")
        LM_SYM(Recv, "ncclRecv")
        LM_SYM(GroupStart, "ncclGroupStart")
        LM_SYM(GroupEnd, "ncclGroupEnd")
        LM_SYM(GetErrorString, "ncclGetErrorString")
        LM_SYM(GetVersion, "ncclGetVersion")
#undef LM_SYM
        // 2.7.0 is 2700 in the old numbering (major * 1000 + minor * 100 + patch), 2.9+ count major * 10000: both are >= 2700
        if (r.GetVersion(&r.version) != ncclSuccess || r.version < 2700) {
            r.err = "the RCCL that was found is older than 2.7 (no ncclSend / ncclRecv): version code " + std::to_string(r.version);
            return;
        }
        r.ok = true;
    });
    return r;
}
} // namespace

struct lm_comm {
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0, device = 0;
    hipStream_t st = nullptr;
    // grow-only staging: device send / receive buffers, pinned host mirror of the received rows, the counts
    void *d_send = nullptr, *d_recv = nullptr, *h_recv = nullptr, *h_send = nullptr;
    size_t send_cap = 0, recv_cap = 0, hrecv_cap = 0, hsend_cap = 0;
    unsigned long long *d_counts = nullptr; // [4 (nranks + 1)]: the gathered {rows, string bytes, flags | status}, then this rank's own
    std::vector<size_t> counts;
    // lm_gather_merge_rows: all ranks' rows in rank order, the merged rows, their pinned host mirror, the merge's scratch
    void *d_all = nullptr, *d_merged = nullptr, *h_merged = nullptr;
    size_t all_cap = 0, merged_cap = 0, hmerged_cap = 0;
    lm::MergeScratch ms;
    // the string columns (LM_ROW_ALL): lengths + blocks of lm_gather_rows_ex's rows (pinned); lengths + blocks of all ranks on the
    // device (lm_gather_merge_rows_ex without a handle); the merged blocks on the device and their pinned host mirror
    void *h_str = nullptr, *d_str = nullptr, *d_mstr = nullptr, *h_mstr = nullptr;
    size_t hstr_cap = 0, dstr_cap = 0, dmstr_cap = 0, hmstr_cap = 0;
    std::string err;
    std::mutex mu;
};

static_assert(sizeof(ncclUniqueId) == LM_COMM_ID_BYTES, "lm_comm_unique_id hands out an ncclUniqueId");

#define CK_HIP(c, expr)                                                                                \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (c)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                              \
            return LM_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)
#define CK_NCCL(c, expr)                                                                               \
    do {                                                                                               \
        ncclResult_t e_ = (expr);                                                                      \
        if (e_ != ncclSuccess) {                                                                       \
            (c)->err = std::string(#expr) + ": " + rccl().GetErrorString(e_);                          \
            return LM_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)

extern "C" {

lm_status lm_comm_unique_id(uint8_t id[LM_COMM_ID_BYTES]) {
    if (!id) return LM_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        g_open_error = "no HIP device: the row gather runs over RCCL between GPUs";
        return LM_ERR_NO_DEVICE;
    }
    Rccl &r = rccl();
    if (!r.ok) {
        g_open_error = r.err;
        return LM_ERR_HIP;
    }
    ncclUniqueId u;
    ncclResult_t e = r.GetUniqueId(&u);
    if (e != ncclSuccess) {
        g_open_error = std::string("ncclGetUniqueId: ") + r.GetErrorString(e);
        return LM_ERR_HIP;
    }
    memcpy(id, &u, LM_COMM_ID_BYTES);
    return LM_OK;
}

lm_status lm_comm_init(const uint8_t id[LM_COMM_ID_BYTES], int nranks, int rank, int device, lm_comm **out) {
    if (!out) return LM_ERR_ARG;
    *out = nullptr;
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return LM_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        g_open_error = "no HIP device: the row gather runs over RCCL between GPUs";
        return LM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        g_open_error = "lm_comm_init: no such device";
        return LM_ERR_ARG;
    }
    Rccl &r = rccl();
    if (!r.ok) {
        g_open_error = r.err;
        return LM_ERR_HIP;
    }
    lm_comm *c = new lm_comm();
    c->nranks = nranks;
    c->rank = rank;
    c->device = device;
    c->counts.assign((size_t)nranks, 0);
    auto fail = [&](const std::string &m) {
        g_open_error = m;
        lm_comm_free(c);
        return LM_ERR_HIP;
    };
    if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed");
    ncclUniqueId u;
    memcpy(&u, id, LM_COMM_ID_BYTES);
    ncclResult_t e = r.CommInitRank(&c->comm, nranks, u, rank);
    if (e != ncclSuccess) {
        c->comm = nullptr;
        return fail(std::string("ncclCommInitRank: ") + r.GetErrorString(e));
    }
    if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
    if (hipMalloc((void **)&c->d_counts, sizeof(unsigned long long) * 4 * (size_t)(nranks + 1)) != hipSuccess) return fail("hipMalloc failed");
    *out = c;
    return LM_OK;
}

void lm_comm_free(lm_comm *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->st) (void)hipStreamSynchronize(c->st);
    if (c->comm && rccl().ok) (void)rccl().CommDestroy(c->comm);
    if (c->d_send) (void)hipFree(c->d_send);
    if (c->d_recv) (void)hipFree(c->d_recv);
    if (c->d_counts) (void)hipFree(c->d_counts);
    if (c->h_recv) (void)hipHostFree(c->h_recv);
    if (c->h_send) (void)hipHostFree(c->h_send);
    if (c->d_all) (void)hipFree(c->d_all);
    if (c->d_merged) (void)hipFree(c->d_merged);
    if (c->h_merged) (void)hipHostFree(c->h_merged);
    if (c->h_str) (void)hipHostFree(c->h_str);
    if (c->d_str) (void)hipFree(c->d_str);
    if (c->d_mstr) (void)hipFree(c->d_mstr);
    if (c->h_mstr) (void)hipHostFree(c->h_mstr);
    c->ms.release();
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
}

const char *lm_comm_last_error(const lm_comm *c) { return c ? c->err.c_str() : g_open_error.c_str(); }
int lm_comm_rank(const lm_comm *c) { return c ? c->rank : -1; }
int lm_comm_size(const lm_comm *c) { return c ? c->nranks : 0; }

static lm_status grow_dev(lm_comm *c, void **p, size_t *cap, size_t need) {
    if (need <= *cap && *p) return LM_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = need + need / 4 + 4096;
    CK_HIP(c, hipMalloc(p, want));
    *cap = want;
    return LM_OK;
}
static lm_status grow_host(lm_comm *c, void **p, size_t *cap, size_t need) {
    if (need <= *cap && *p) return LM_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = need + need / 4 + 4096;
    CK_HIP(c, hipHostMalloc(p, want, hipHostMallocDefault));
    *cap = want;
    return LM_OK;
}

} // extern "C"

// ---- the string columns on the wire (lm_merge.h; LM_ROW_ALL) ---------------------------------------------------------------
// host threads over [0, n) in up to 8 contiguous parts, the same parts for the same n: f(part, begin, end); returns the parts
template <class F> static int host_parts(size_t n, F f) {
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    const int np = (int)std::min<size_t>((size_t)std::min(8, hw), std::max<size_t>(1, n / 16384));
    std::vector<std::thread> th;
    for (int p = 1; p < np; p++) th.emplace_back([&, p] { f(p, n * (size_t)p / (size_t)np, n * (size_t)(p + 1) / (size_t)np); });
    f(0, 0, n / (size_t)np);
    for (auto &t : th) t.join();
    return np;
}
// lens[4 n] of rows' strings; returns the bytes of their blocks, or UINT64_MAX when a string is too long for a uint32 length
static uint64_t wire_lens(const lm_hsp *rows, size_t n, uint32_t *lens) {
    uint64_t part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool bad[8] = {false, false, false, false, false, false, false, false};
    const int np = host_parts(n, [&](int p, size_t b, size_t e) {
        uint64_t sum = 0;
        for (size_t i = b; i < e; i++) {
            const char *str[4] = {rows[i].cigar, rows[i].qseq, rows[i].sseq, rows[i].align};
            for (int k = 0; k < 4; k++) {
                const size_t l = str[k] ? strlen(str[k]) : (size_t)lm::kStrNull;
                if (str[k] && l >= (size_t)lm::kStrNull) bad[p] = true;
                lens[4 * i + (size_t)k] = (uint32_t)l;
            }
            sum += lm::block_bytes(lens + 4 * i);
        }
        part[p] = sum;
    });
    uint64_t total = 0;
    for (int p = 0; p < np; p++) {
        if (bad[p]) return UINT64_MAX;
        total += part[p];
    }
    return total;
}
// start of every part's blocks (the parts of host_parts(n)), from the lengths
static int wire_parts(size_t n, const uint32_t *lens, uint64_t at[9]) {
    uint64_t part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int np = host_parts(n, [&](int p, size_t b, size_t e) {
        uint64_t sum = 0;
        for (size_t i = b; i < e; i++) sum += lm::block_bytes(lens + 4 * i);
        part[p] = sum;
    });
    at[0] = 0;
    for (int p = 0; p < np; p++) at[p + 1] = at[p] + part[p];
    return np;
}
// the blocks of rows' strings, back to back into blob (lens from wire_lens)
static void wire_fill(const lm_hsp *rows, size_t n, const uint32_t *lens, char *blob) {
    uint64_t at[9];
    wire_parts(n, lens, at);
    host_parts(n, [&](int p, size_t b, size_t e) {
        char *d = blob + at[p];
        for (size_t i = b; i < e; i++) {
            const uint32_t *l = lens + 4 * i;
            const char *str[4] = {rows[i].cigar, rows[i].qseq, rows[i].sseq, rows[i].align};
            char *const d0 = d;
            for (int k = 0; k < 4; k++) {
                if (l[k] == lm::kStrNull) continue;
                memcpy(d, str[k], l[k]);
                d[l[k]] = 0;
                d += l[k] + 1;
            }
            const size_t pad = (size_t)(d0 + lm::block_bytes(l) - d);
            memset(d, 0, pad);
            d += pad;
        }
    });
}
// rows' string pointers into blob (the blocks of the same rows, lens their lengths)
static void wire_attach(lm_hsp *rows, size_t n, const uint32_t *lens, const char *blob) {
    uint64_t at[9];
    wire_parts(n, lens, at);
    host_parts(n, [&](int p, size_t b, size_t e) {
        const char *d = blob + at[p];
        for (size_t i = b; i < e; i++) {
            const uint32_t *l = lens + 4 * i;
            const char **dst[4] = {&rows[i].cigar, &rows[i].qseq, &rows[i].sseq, &rows[i].align};
            const char *q = d;
            for (int k = 0; k < 4; k++) {
                *dst[k] = l[k] == lm::kStrNull ? nullptr : q;
                q += lm::str_bytes(l[k]);
            }
            d += lm::block_bytes(l);
        }
    });
}

// ---- the gather ----------------------------------------------------------------------------------------------------------
// What every rank knows after the count exchange.
struct Counts {
    std::vector<unsigned long long> rows, bytes;
    std::vector<int64_t> off;   // [N + 1] first row of every rank
    std::vector<uint64_t> boff; // [N + 1] first block byte of every rank
    size_t total = 0;
    uint64_t total_bytes = 0;
};
// This rank's payload staged in the pinned h_send: its rows, then (strs) their lengths at n * 168, then their blocks at n * 184.
// With `to_device` the device buffer of the send is grown too.  Errors are returned, not acted on: they go into the count exchange.
static lm_status stage_payload(lm_comm *c, const lm_hsp *rows, size_t n, bool strs, bool to_device, uint64_t *bytes) {
    *bytes = 0;
    if (n == 0) return LM_OK;
    const size_t item = sizeof(lm_hsp);
    std::vector<uint32_t> lens;
    if (strs) {
        lens.resize(4 * n);
        *bytes = wire_lens(rows, n, lens.data());
        if (*bytes == UINT64_MAX) {
            *bytes = 0;
            c->err = "a string column is longer than 4 GB";
            return LM_ERR_ARG;
        }
    }
    const size_t stage = n * item + (strs ? n * 16 + (size_t)*bytes : 0);
    lm_status s = grow_host(c, &c->h_send, &c->hsend_cap, stage); // pinned: the upload is one DMA
    if (s == LM_OK && to_device) s = grow_dev(c, &c->d_send, &c->send_cap, stage);
    if (s != LM_OK) return s == LM_ERR_HIP ? LM_ERR_NOMEM : s;
    memcpy(c->h_send, rows, n * item);
    if (strs) {
        memcpy((char *)c->h_send + n * item, lens.data(), n * 16);
        wire_fill(rows, n, lens.data(), (char *)c->h_send + n * (item + 16));
    }
    return LM_OK;
}
// The count exchange: one all-gather of {rows, string bytes, flags << 8 | status} per rank.  LM_OK when every rank staged its
// payload and all passed the same valid flags; otherwise every rank returns the same kind of error.
static lm_status exchange_counts(lm_comm *c, size_t n, uint64_t bytes, int flags, lm_status mine, Counts &x) {
    Rccl &r = rccl();
    const int N = c->nranks;
    const unsigned long long w[3] = {(unsigned long long)n, (unsigned long long)bytes,
                                     ((unsigned long long)(unsigned)flags << 8) | (unsigned long long)(unsigned)(mine & 0xff)};
    CK_HIP(c, hipMemcpyAsync(c->d_counts + 3 * N, w, sizeof w, hipMemcpyHostToDevice, c->st));
    CK_NCCL(c, r.AllGather(c->d_counts + 3 * N, c->d_counts, 3, ncclUint64, c->comm, c->st));
    std::vector<unsigned long long> all(3 * (size_t)N);
    CK_HIP(c, hipMemcpyAsync(all.data(), c->d_counts, sizeof(unsigned long long) * 3 * (size_t)N, hipMemcpyDeviceToHost, c->st));
    CK_HIP(c, hipStreamSynchronize(c->st));
    x.rows.assign((size_t)N, 0);
    x.bytes.assign((size_t)N, 0);
    x.off.assign((size_t)N + 1, 0);
    x.boff.assign((size_t)N + 1, 0);
    lm_status bad = LM_OK;
    for (int i = 0; i < N; i++) {
        x.rows[(size_t)i] = all[3 * (size_t)i];
        x.bytes[(size_t)i] = all[3 * (size_t)i + 1];
        x.off[(size_t)i + 1] = x.off[(size_t)i] + (int64_t)x.rows[(size_t)i];
        x.boff[(size_t)i + 1] = x.boff[(size_t)i] + x.bytes[(size_t)i];
        const int st = (int)(all[3 * (size_t)i + 2] & 0xff), fl = (int)(all[3 * (size_t)i + 2] >> 8);
        if (bad == LM_OK && st != LM_OK) {
            bad = st;
            if (mine == LM_OK) c->err = "rank " + std::to_string(i) + " could not stage its rows (status " + std::to_string(st) + ")";
        }
        if (bad == LM_OK && (fl != flags || (fl & ~LM_ROW_ALL))) {
            bad = LM_ERR_ARG;
            c->err = "the ranks passed different flags (rank " + std::to_string(i) + ": " + std::to_string(fl) + ", this rank: " + std::to_string(flags) +
                     ") or a flag other than LM_ROW_ALL";
        }
    }
    x.total = (size_t)x.off[(size_t)N];
    x.total_bytes = x.boff[(size_t)N];
    return bad;
}
// The root's go / no-go once it has sized and allocated everything it receives into: a second all-gather (8 bytes per rank),
// so that no rank sends to a root that has returned.
static lm_status root_go(lm_comm *c, int root, lm_status mine) {
    Rccl &r = rccl();
    const int N = c->nranks;
    const unsigned long long w = c->rank == root ? (unsigned long long)(unsigned)mine : 0ull;
    CK_HIP(c, hipMemcpyAsync(c->d_counts + 3 * N, &w, sizeof w, hipMemcpyHostToDevice, c->st));
    CK_NCCL(c, r.AllGather(c->d_counts + 3 * N, c->d_counts, 1, ncclUint64, c->comm, c->st));
    unsigned long long go = 0;
    CK_HIP(c, hipMemcpyAsync(&go, c->d_counts + root, sizeof go, hipMemcpyDeviceToHost, c->st));
    CK_HIP(c, hipStreamSynchronize(c->st));
    if (go == 0) return LM_OK;
    if (c->rank != root) c->err = "the root could not allocate what it receives into (status " + std::to_string(go) + ")";
    return mine != LM_OK ? mine : LM_ERR_NOMEM;
}
// A rank that does not merge: its staged payload (stage_payload with to_device) to the device in one DMA, then one group of
// sends - rows, lengths, blocks - to the root.
static lm_status send_payload(lm_comm *c, int root, size_t n, bool strs, uint64_t bytes) {
    Rccl &r = rccl();
    const size_t item = sizeof(lm_hsp);
    if (n > 0) {
        const size_t stage = n * item + (strs ? n * 16 + (size_t)bytes : 0);
        CK_HIP(c, hipMemcpyAsync(c->d_send, c->h_send, stage, hipMemcpyHostToDevice, c->st));
        CK_NCCL(c, r.GroupStart());
        ncclResult_t e = r.Send(c->d_send, n * item, ncclUint8, root, c->comm, c->st);
        if (e == ncclSuccess && strs) e = r.Send((char *)c->d_send + n * item, n * 16, ncclUint8, root, c->comm, c->st);
        if (e == ncclSuccess && strs && bytes > 0) e = r.Send((char *)c->d_send + n * (item + 16), (size_t)bytes, ncclUint8, root, c->comm, c->st);
        if (e != ncclSuccess) {
            (void)r.GroupEnd();
            c->err = std::string("ncclSend: ") + r.GetErrorString(e);
            return LM_ERR_HIP;
        }
        CK_NCCL(c, r.GroupEnd());
    }
    CK_HIP(c, hipStreamSynchronize(c->st));
    return LM_OK;
}
// The root: one group of receives, from every other rank its rows at rows + off[i] * 168, (strs) its lengths at lens + off[i] * 16
// and its blocks at blob + boff[i].  With `packed` the rows / lengths / blocks of the other ranks land back to back without gaps
// for the root's own (lm_gather_rows_ex: a device staging area downloaded afterwards).
static lm_status recv_payloads(lm_comm *c, int root, const Counts &x, bool strs, char *rows, char *lens, char *blob, bool packed) {
    Rccl &r = rccl();
    const size_t item = sizeof(lm_hsp);
    if (x.total == (size_t)x.rows[(size_t)root]) return LM_OK;
    CK_NCCL(c, r.GroupStart());
    int64_t skip = 0;
    uint64_t bskip = 0;
    for (int i = 0; i < c->nranks; i++) {
        const size_t n = (size_t)x.rows[(size_t)i];
        if (i == root) {
            if (packed) {
                skip = (int64_t)n;
                bskip = x.bytes[(size_t)i];
            }
            continue;
        }
        if (n == 0) continue;
        const size_t at = (size_t)(x.off[(size_t)i] - (i > root ? skip : 0));
        const uint64_t bat = x.boff[(size_t)i] - (i > root ? bskip : 0);
        ncclResult_t e = r.Recv(rows + at * item, n * item, ncclUint8, i, c->comm, c->st);
        if (e == ncclSuccess && strs) e = r.Recv(lens + at * 16, n * 16, ncclUint8, i, c->comm, c->st);
        if (e == ncclSuccess && strs && x.bytes[(size_t)i] > 0) e = r.Recv(blob + bat, (size_t)x.bytes[(size_t)i], ncclUint8, i, c->comm, c->st);
        if (e != ncclSuccess) {
            (void)r.GroupEnd();
            c->err = std::string("ncclRecv: ") + r.GetErrorString(e);
            return LM_ERR_HIP;
        }
    }
    CK_NCCL(c, r.GroupEnd());
    return LM_OK;
}

extern "C" {

// rows / n: this rank's rows (host memory, as lm_result_rows returns them).  On `root`: *all_rows = the rows of rank 0,
// then rank 1, ... (nrows[r] of each; genome_id / seq_id cleared - they are addresses of another process - and the string
// columns cleared, or with LM_ROW_ALL pointing into the communicator's pinned h_str), valid until the next call on this
// communicator; on the other ranks *all_rows = NULL and nrows[] still holds every rank's count.
lm_status lm_gather_rows_ex(lm_comm *c, const lm_hsp *rows, size_t n, int root, int flags, const lm_hsp **all_rows, size_t *nrows) {
    if (!c || !all_rows || !nrows || (n > 0 && !rows) || root < 0 || root >= c->nranks) return LM_ERR_ARG;
    *all_rows = nullptr;
    std::lock_guard<std::mutex> lock(c->mu);
    CK_HIP(c, hipSetDevice(c->device));
    const int N = c->nranks;
    const bool strs = (flags & LM_ROW_ALL) != 0;
    const size_t item = sizeof(lm_hsp);
    // 1. the payload of a rank that sends, staged before the exchange (a failure travels with the counts); the counts
    uint64_t mybytes = 0;
    lm_status mine = LM_OK;
    if (c->rank != root) mine = stage_payload(c, rows, n, strs, true, &mybytes);
    else if (strs && n > 0) { // (the root only needs the size of its blocks here; they are written in place below)
        std::vector<uint32_t> l(4 * n);
        mybytes = wire_lens(rows, n, l.data());
        if (mybytes == UINT64_MAX) {
            mybytes = 0;
            c->err = "a string column is longer than 4 GB";
            mine = LM_ERR_ARG;
        }
    }
    Counts x;
    lm_status s = exchange_counts(c, n, mybytes, flags, mine, x);
    if (s != LM_OK) return s;
    for (int i = 0; i < N; i++) nrows[i] = (size_t)x.rows[(size_t)i];
    // 2. the payloads: the root keeps its own rows on the host; every other rank sends from the device
    if (c->rank != root) {
        if (strs && x.total > 0) {
            s = root_go(c, root, LM_OK);
            if (s != LM_OK) return s;
        }
        return send_payload(c, root, n, strs, mybytes);
    }
    const size_t total = x.total, remote = total - n;
    const uint64_t rbytes = x.total_bytes - mybytes;
    // remote rows | remote lengths | remote blocks (16-byte aligned) in one device area
    const size_t lens_at = (remote * item + 15) & ~(size_t)15, blob_at = lens_at + (strs ? remote * 16 : 0);
    s = grow_host(c, &c->h_recv, &c->hrecv_cap, std::max<size_t>(total, 1) * item);
    if (s == LM_OK && strs) s = grow_host(c, &c->h_str, &c->hstr_cap, total * 16 + (size_t)x.total_bytes + 16);
    if (s == LM_OK && remote > 0) s = grow_dev(c, &c->d_recv, &c->recv_cap, blob_at + (strs ? (size_t)rbytes : 0));
    if (strs && total > 0) {
        const lm_status go = root_go(c, root, s);
        if (go != LM_OK) return s != LM_OK ? s : go;
    } else if (s != LM_OK)
        return s;
    char *const d = (char *)c->d_recv;
    s = recv_payloads(c, root, x, strs, d, d + lens_at, d + blob_at, true);
    if (s != LM_OK) return s;
    char *const h_lens = (char *)c->h_str, *const h_blob = strs ? (char *)c->h_str + total * 16 : nullptr;
    if (remote > 0) { // device -> the pinned host mirrors, every rank's part at its place in rank order
        int64_t skip = 0;
        uint64_t bskip = 0;
        for (int i = 0; i < N; i++) {
            const size_t ni = nrows[i];
            if (i == root) {
                skip = (int64_t)ni;
                bskip = x.bytes[(size_t)i];
                continue;
            }
            if (ni == 0) continue;
            const size_t at = (size_t)(x.off[(size_t)i] - (i > root ? skip : 0));
            CK_HIP(c, hipMemcpyAsync((char *)c->h_recv + (size_t)x.off[(size_t)i] * item, d + at * item, ni * item, hipMemcpyDeviceToHost, c->st));
            if (strs) {
                CK_HIP(c, hipMemcpyAsync(h_lens + (size_t)x.off[(size_t)i] * 16, d + lens_at + at * 16, ni * 16, hipMemcpyDeviceToHost, c->st));
                if (x.bytes[(size_t)i] > 0)
                    CK_HIP(c, hipMemcpyAsync(h_blob + x.boff[(size_t)i], d + blob_at + (x.boff[(size_t)i] - (i > root ? bskip : 0)), (size_t)x.bytes[(size_t)i],
                                             hipMemcpyDeviceToHost, c->st));
            }
        }
    }
    if (n > 0) { // (beside the transfers)
        memcpy((char *)c->h_recv + (size_t)x.off[(size_t)root] * item, rows, n * item);
        if (strs) {
            uint32_t *ml = (uint32_t *)(h_lens + (size_t)x.off[(size_t)root] * 16);
            (void)wire_lens(rows, n, ml);
            wire_fill(rows, n, ml, h_blob + x.boff[(size_t)root]);
        }
    }
    CK_HIP(c, hipStreamSynchronize(c->st));
    lm_hsp *all = (lm_hsp *)c->h_recv;
    for (size_t i = 0; i < total; i++) { // addresses of another process (and of results the caller may free)
        all[i].genome_id = nullptr;
        all[i].seq_id = nullptr;
        all[i].cigar = nullptr;
        all[i].qseq = nullptr;
        all[i].sseq = nullptr;
        all[i].align = nullptr;
    }
    if (strs) wire_attach(all, total, (const uint32_t *)h_lens, h_blob);
    *all_rows = all;
    return LM_OK;
}
lm_status lm_gather_rows(lm_comm *c, const lm_hsp *rows, size_t n, int root, const lm_hsp **all_rows, size_t *nrows) {
    return lm_gather_rows_ex(c, rows, n, root, 0, all_rows, nrows);
}

// the handle's idle scratch slabs as the allocator of one merge (lm_merge.h)
static void *borrow_cb(void *ctx, size_t bytes) { return lm_scratch_borrow((lm_index *)ctx, bytes); }
static void return_cb(void *ctx, void *p) { lm_scratch_return((lm_index *)ctx, p); }

// The string columns of a device merge: lengths (4 per row) and blocks of all rows in device memory, rank order.
struct StrIn {
    const uint32_t *lens;
    const char *blob;
    uint64_t bytes;
};

// rows of all shards in device memory, rank order -> the final order in the communicator's pinned buffer (lm_merge.hip + one
// download + the names); with `si` the blocks of the strings follow their rows into h_mstr (a second download).  The caller holds
// c->mu and, when idx is given, the handle's scratch session (the buffers of the merge are then borrowed from the handle's
// scratch slabs)
static lm_status merge_on_device(lm_comm *c, lm_index *idx, const lm_hsp *d_rows, const int64_t *off, int N, const StrIn *si, const lm_hsp **merged,
                                 size_t *total_out) {
    const size_t total = (size_t)off[N], item = sizeof(lm_hsp);
    const uint64_t sbytes = si ? si->bytes : 0;
    lm_status s = grow_host(c, &c->h_merged, &c->hmerged_cap, total * item);
    if (s == LM_OK && si) s = grow_host(c, &c->h_mstr, &c->hmstr_cap, (size_t)sbytes + 16);
    if (s != LM_OK) return s;
    lm_hsp *d_out = nullptr;
    char *d_mstr = nullptr;
    if (idx) {
        c->ms.borrow = borrow_cb;
        c->ms.give_back = return_cb;
        c->ms.ctx = idx;
        d_out = (lm_hsp *)c->ms.take(total * item);
        if (d_out && sbytes > 0) d_mstr = (char *)c->ms.take((size_t)sbytes);
        if (!d_out || (sbytes > 0 && !d_mstr)) {
            c->ms.end_call();
            c->err = "the merge's buffers do not fit the index handle's scratch";
            return LM_ERR_NOMEM;
        }
    } else {
        s = grow_dev(c, &c->d_merged, &c->merged_cap, total * item);
        if (s == LM_OK && sbytes > 0) s = grow_dev(c, &c->d_mstr, &c->dmstr_cap, (size_t)sbytes);
        if (s != LM_OK) return s;
        d_out = (lm_hsp *)c->d_merged;
        d_mstr = (char *)c->d_mstr;
    }
    lm::MergeStrings ms;
    if (si) {
        ms.lens = si->lens;
        ms.in = si->blob;
        ms.out = d_mstr;
        ms.bytes = sbytes;
        ms.host = (uint64_t)(uintptr_t)c->h_mstr;
    }
    const bool dbg = getenv("LM_DEBUG") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    hipError_t e = lm::merge_rows_device(c->st, d_rows, total, off, N, d_out, c->ms, si ? &ms : nullptr);
    if (e == hipSuccess && dbg) e = hipStreamSynchronize(c->st);
    const double t1 = now();
    // the rows and the blocks: two DMAs on the communicator's stream
    if (e == hipSuccess) e = hipMemcpyAsync(c->h_merged, d_out, total * item, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess && sbytes > 0) e = hipMemcpyAsync(c->h_mstr, d_mstr, (size_t)sbytes, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    else (void)hipStreamSynchronize(c->st);
    c->ms.end_call(); // (borrowed buffers go back to the handle whatever happened)
    if (e != hipSuccess) {
        if (si && e == hipErrorInvalidValue) {
            c->err = "device merge: the string lengths do not add up to the bytes of the blocks";
            return LM_ERR_ARG;
        }
        c->err = std::string("device merge: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? LM_ERR_NOMEM : LM_ERR_HIP;
    }
    const double t2 = now();
    lm_attach_names(idx, (lm_hsp *)c->h_merged, total);
    if (dbg)
        fprintf(stderr, "[lm] device merge of %zu rows: order %.1f ms, download %.1f ms (%.1f GB/s), names %.1f ms\n", total, t1 - t0, t2 - t1,
                (double)(total * item + sbytes) / 1e6 / std::max(t2 - t1, 1e-3), now() - t2);
    *merged = (const lm_hsp *)c->h_merged;
    *total_out = total;
    return LM_OK;
}

// The gather and the merge in one call: the rows of the other ranks are received into device memory at their place in rank order,
// this rank's own rows are uploaded beside them, the final order is made on the device (lm_merge.hip) and downloaded ONCE into
// the communicator's pinned buffer; the names are re-attached by the host threads.  Same rows, same order, same `hits` as
// lm_gather_rows + lm_merge_sharded.  On `root`: *merged / *total; elsewhere *merged = NULL, *total = 0.  idx (may be NULL:
// names stay NULL) is the root's index handle.  All ranks call it, in the same order as their other collective calls.  With
// LM_ROW_ALL the lengths and blocks of the strings travel and are reordered beside the rows (lm_merge.hip).
lm_status lm_gather_merge_rows_ex(lm_comm *c, lm_index *idx, const lm_hsp *rows, size_t n, int root, int flags, const lm_hsp **merged, size_t *total_out) {
    if (!c || !merged || !total_out || (n > 0 && !rows) || root < 0 || root >= c->nranks) return LM_ERR_ARG;
    *merged = nullptr;
    *total_out = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    CK_HIP(c, hipSetDevice(c->device));
    const int N = c->nranks;
    const bool strs = (flags & LM_ROW_ALL) != 0;
    const size_t item = sizeof(lm_hsp);
    // this rank's rows (and strings) through the pinned mirror (one DMA): the payload of a send, or the root's own part
    uint64_t mybytes = 0;
    const lm_status mine = stage_payload(c, rows, n, strs, c->rank != root, &mybytes);
    Counts x;
    lm_status s = exchange_counts(c, n, mybytes, flags, mine, x);
    if (s != LM_OK) return s;
    const size_t total = x.total;
    if (c->rank != root) {
        if (strs && total > 0) {
            s = root_go(c, root, LM_OK);
            if (s != LM_OK) return s;
        }
        return send_payload(c, root, n, strs, mybytes);
    }
    if (total == 0) return LM_OK;
    // the gathered rows (and lengths + blocks): in the handle's scratch when there is one (idle between two searches), else in
    // buffers of the communicator
    struct Session {
        lm_index *ix;
        void *blk[2] = {nullptr, nullptr};
        explicit Session(lm_index *i) : ix(i) {
            if (ix) lm_scratch_session_begin(ix);
        }
        ~Session() {
            for (void *b : blk)
                if (ix && b) lm_scratch_return(ix, b);
            if (ix) lm_scratch_session_end(ix);
        }
    } session(idx);
    const size_t str_need = strs ? total * 16 + (size_t)x.total_bytes : 0;
    if (idx) {
        session.blk[0] = lm_scratch_borrow(idx, total * item);
        if (session.blk[0] && strs) session.blk[1] = lm_scratch_borrow(idx, str_need);
        s = session.blk[0] && (!strs || session.blk[1]) ? LM_OK : LM_ERR_NOMEM;
        if (s != LM_OK) c->err = "the gathered rows do not fit the index handle's scratch";
    } else {
        s = grow_dev(c, &c->d_all, &c->all_cap, total * item);
        if (s == LM_OK && strs) s = grow_dev(c, &c->d_str, &c->dstr_cap, str_need);
    }
    if (strs) { // everything the root receives into or downloads into, before the go / no-go
        if (s == LM_OK) s = grow_host(c, &c->h_merged, &c->hmerged_cap, total * item);
        if (s == LM_OK) s = grow_host(c, &c->h_mstr, &c->hmstr_cap, (size_t)x.total_bytes + 16);
        const lm_status go = root_go(c, root, s);
        if (s != LM_OK || go != LM_OK) return s != LM_OK ? s : go;
    } else if (s != LM_OK) {
        // (the other ranks are sending: receive into nothing is not possible - the job fails, as any error inside a collective)
        return s;
    }
    char *const d_all = idx ? (char *)session.blk[0] : (char *)c->d_all;
    char *const d_str = strs ? (idx ? (char *)session.blk[1] : (char *)c->d_str) : nullptr;
    char *const d_lens = d_str, *const d_blob = strs ? d_str + total * 16 : nullptr;
    if (n > 0) {
        CK_HIP(c, hipMemcpyAsync(d_all + (size_t)x.off[(size_t)root] * item, c->h_send, n * item, hipMemcpyHostToDevice, c->st));
        if (strs) {
            CK_HIP(c, hipMemcpyAsync(d_lens + (size_t)x.off[(size_t)root] * 16, (char *)c->h_send + n * item, n * 16, hipMemcpyHostToDevice, c->st));
            if (mybytes > 0)
                CK_HIP(c, hipMemcpyAsync(d_blob + x.boff[(size_t)root], (char *)c->h_send + n * (item + 16), (size_t)mybytes, hipMemcpyHostToDevice, c->st));
        }
    }
    s = recv_payloads(c, root, x, strs, d_all, d_lens, d_blob, false);
    if (s != LM_OK) return s;
    const StrIn si{(const uint32_t *)d_lens, d_blob, x.total_bytes};
    return merge_on_device(c, idx, (const lm_hsp *)d_all, x.off.data(), N, strs ? &si : nullptr, merged, total_out);
}
lm_status lm_gather_merge_rows(lm_comm *c, lm_index *idx, const lm_hsp *rows, size_t n, int root, const lm_hsp **merged, size_t *total_out) {
    return lm_gather_merge_rows_ex(c, idx, rows, n, root, 0, merged, total_out);
}

// What the merging rank does once the rows have arrived, by itself: `d_rows` = the rows of shard 0, 1, ... back to back IN DEVICE
// MEMORY (nrows[r] of each; each block grouped by query ascending, a genome's rows together), merged on the device on the
// communicator's stream (a single-rank communicator will do), downloaded once, names re-attached from idx.  *merged as in
// lm_gather_merge_rows.  (bench.py times the merge of N shards' worth of rows on one GPU with it.)  With LM_ROW_ALL, d_strings
// holds the lengths and blocks of the same rows in the wire form (include/lexicmap_hip.h).
lm_status lm_merge_sharded_device_ex(lm_comm *c, lm_index *idx, const void *d_rows, const size_t *nrows, const void *d_strings, uint64_t string_bytes,
                                     int nshards, int flags, const lm_hsp **merged, size_t *total_out) {
    if (!c || !merged || !total_out || !nrows || nshards < 1 || (flags & ~LM_ROW_ALL)) return LM_ERR_ARG;
    *merged = nullptr;
    *total_out = 0;
    const bool strs = (flags & LM_ROW_ALL) != 0;
    std::lock_guard<std::mutex> lock(c->mu);
    CK_HIP(c, hipSetDevice(c->device));
    std::vector<int64_t> off((size_t)nshards + 1, 0);
    for (int i = 0; i < nshards; i++) off[(size_t)i + 1] = off[(size_t)i] + (int64_t)nrows[i];
    const size_t total = (size_t)off[(size_t)nshards];
    if (total == 0) return LM_OK;
    if (!d_rows) return LM_ERR_ARG;
    if (strs && (!d_strings || ((uintptr_t)d_strings & 15) != 0)) {
        c->err = "lm_merge_sharded_device_ex: d_strings must be a 16-byte aligned device address";
        return LM_ERR_ARG;
    }
    const StrIn si{(const uint32_t *)d_strings, strs ? (const char *)d_strings + total * 16 : nullptr, string_bytes};
    if (idx) lm_scratch_session_begin(idx);
    const lm_status st = merge_on_device(c, idx, (const lm_hsp *)d_rows, off.data(), nshards, strs ? &si : nullptr, merged, total_out);
    if (idx) lm_scratch_session_end(idx);
    return st;
}
lm_status lm_merge_sharded_device(lm_comm *c, lm_index *idx, const void *d_rows, const size_t *nrows, int nshards, const lm_hsp **merged,
                                  size_t *total_out) {
    return lm_merge_sharded_device_ex(c, idx, d_rows, nrows, nullptr, 0, nshards, 0, merged, total_out);
}

} // extern "C"
