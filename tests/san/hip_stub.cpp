// tests/san/hip_stub.cpp — TEST INFRASTRUCTURE ONLY: a host-memory stand-in for the HIP / RCCL
// runtime calls engine.cpp makes, so the C ABI's host side can be built and run on a CPU.
// "Device" memory is host memory, copies are memcpy, every call completes before it returns
// (so stream and event order hold trivially) and events carry a host timestamp.
//
// Two builds (never shipped, never loaded by the product path):
//   * default (tests/test_sanitize.py, tests/test_family_host.py): the kernel launchers compute
//     nothing but read their inputs and write patterns over their outputs (see "kernel launchers"
//     below); engine.cpp's argument validation, staging and error paths run under ASan + UBSan.
// Every launcher and scratch-size function of kernels.hpp has its stand-in here, in both builds
// (MPX_STUB_ORACLE only changes the group step), so engine.cpp links with no symbol left open.
//   * -DMPX_STUB_ORACLE=1 (tests/test_dist.py, libmpx_stub.so): the group-step launchers run the
//     CPU oracle (oracle/oracle.cpp, linked into the stub) and the RCCL calls really reduce across
//     PROCESSES — every rank maps one /dev/shm segment named after the unique id, deposits its
//     buffer in its slot, waits at a barrier, and reads the reduction of all slots. That is what
//     lets bench.py's multi-rank step (engine.cpp's nranks > 1 path: comm init, the fused
//     max + sum group, double-buffered watermark vectors) run end to end without a GPU.
// MPX_STUB_DEVICES (default 1) sets the device count the stub reports.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../minpaxos_amd/csrc/kernels.hpp"

namespace {
double now_s() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec + t.tv_nsec * 1e-9;
}

// ---- cross-process communicator: one shared segment per unique id ---------------------------
constexpr size_t kSlotBytes = 64ull << 20;  // per rank (sparse: only touched pages use memory)
constexpr int kMaxRanks = 16;
struct ShmHeader {
    std::atomic<uint32_t> arrived;
    std::atomic<uint32_t> generation;
    std::atomic<uint32_t> joined;
    uint32_t nranks;
};
struct StubComm {
    ShmHeader* hdr = nullptr;
    char* slots = nullptr;
    size_t map_bytes = 0;
    int nranks = 1, rank = 0;
    char name[64] = {0};
};

// sense-reversing barrier over the segment; false after 120 s (a peer died)
bool barrier(StubComm* c) {
    if (c->nranks == 1) return true;
    const uint32_t gen = c->hdr->generation.load(std::memory_order_acquire);
    if (c->hdr->arrived.fetch_add(1, std::memory_order_acq_rel) == (uint32_t)c->nranks - 1) {
        c->hdr->arrived.store(0, std::memory_order_relaxed);
        c->hdr->generation.fetch_add(1, std::memory_order_acq_rel);
        return true;
    }
    const double t0 = now_s();
    while (c->hdr->generation.load(std::memory_order_acquire) == gen) {
        sched_yield();
        if (now_s() - t0 > 120.0) return false;
    }
    return true;
}

template <typename T>
void reduce_into(T* d, const char* slots, int nranks, size_t n, ncclRedOp_t op) {
    for (size_t i = 0; i < n; ++i) {
        T acc = reinterpret_cast<const T*>(slots)[i];
        for (int r = 1; r < nranks; ++r) {
            const T v = reinterpret_cast<const T*>(slots + (size_t)r * kSlotBytes)[i];
            switch (op) {
                case ncclMax: acc = v > acc ? v : acc; break;
                case ncclMin: acc = v < acc ? v : acc; break;
                default: acc = (T)(acc + v); break;
            }
        }
        d[i] = acc;
    }
}

size_t el_size(ncclDataType_t t) {
    switch (t) {
        case ncclInt8: case ncclUint8: return 1;
        case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
        default: return 4;
    }
}

int stub_devices() {
    const char* s = getenv("MPX_STUB_DEVICES");
    const int n = s ? atoi(s) : 1;
    return n > 0 ? n : 1;
}
}  // namespace

extern "C" {
hipError_t hipSetDevice(int d) { return d >= 0 && d < stub_devices() ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetDeviceCount(int* c) { *c = stub_devices(); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
    *s = reinterpret_cast<hipStream_t>(malloc(8));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) { *p = calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
    *p = calloc(1, n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) { *d = h; return hipSuccess; }
hipError_t hipMemset(void* p, int v, size_t n) { memset(p, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
    memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    *e = reinterpret_cast<hipEvent_t>(calloc(1, sizeof(double)));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
    *reinterpret_cast<double*>(e) = now_s();  // the work before it has completed (synchronous)
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    *ms = (float)((*reinterpret_cast<double*>(b) - *reinterpret_cast<double*>(a)) * 1e3);
    return hipSuccess;
}
// graph capture: the stub runs every call at once, so it has nothing to record
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorNotSupported; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t*) { return hipErrorNotSupported; }
hipError_t hipGraphInstantiate(hipGraphExec_t*, hipGraph_t, hipGraphNode_t*, char*, size_t) {
    return hipErrorNotSupported;
}
hipError_t hipGraphDestroy(hipGraph_t) { return hipErrorNotSupported; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipErrorNotSupported; }
hipError_t hipRuntimeGetVersion(int* v) { *v = 1; return hipSuccess; }
hipError_t hipDriverGetVersion(int* v) { *v = 1; return hipSuccess; }

ncclResult_t ncclGetUniqueId(ncclUniqueId* id) {
    memset(id, 0, sizeof(*id));
    int fd = open("/dev/urandom", O_RDONLY);
    if (fd < 0 || read(fd, id->internal, 16) != 16) {
        if (fd >= 0) close(fd);
        return ncclSystemError;
    }
    close(fd);
    return ncclSuccess;
}
ncclResult_t ncclCommInitRank(ncclComm_t* out, int nranks, ncclUniqueId id, int rank) {
    if (nranks < 1 || nranks > kMaxRanks || rank < 0 || rank >= nranks) return ncclInvalidArgument;
    StubComm* c = new StubComm();
    c->nranks = nranks;
    c->rank = rank;
    char* p = c->name + snprintf(c->name, sizeof c->name, "/mpxstub_");
    for (int i = 0; i < 16; ++i) p += sprintf(p, "%02x", (unsigned char)id.internal[i]);
    c->map_bytes = 4096 + (size_t)nranks * kSlotBytes;
    int fd = shm_open(c->name, O_CREAT | O_RDWR, 0600);
    if (fd < 0 || ftruncate(fd, (off_t)c->map_bytes) != 0) {
        if (fd >= 0) close(fd);
        delete c;
        return ncclSystemError;
    }
    void* m = mmap(nullptr, c->map_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (m == MAP_FAILED) {
        delete c;
        return ncclSystemError;
    }
    c->hdr = reinterpret_cast<ShmHeader*>(m);  // a fresh segment is zero-filled
    c->slots = reinterpret_cast<char*>(m) + 4096;
    c->hdr->joined.fetch_add(1);
    if (!barrier(c)) {
        munmap(m, c->map_bytes);
        delete c;
        return ncclSystemError;
    }
    if (rank == 0) shm_unlink(c->name);  // every rank has it mapped: nothing left in /dev/shm
    *out = reinterpret_cast<ncclComm_t>(c);
    return ncclSuccess;
}
ncclResult_t ncclCommDestroy(ncclComm_t h) {
    StubComm* c = reinterpret_cast<StubComm*>(h);
    if (c) {
        munmap(c->hdr, c->map_bytes);
        delete c;
    }
    return ncclSuccess;
}
ncclResult_t ncclAllReduce(const void* s, void* d, size_t n, ncclDataType_t t, ncclRedOp_t op,
                           ncclComm_t h, hipStream_t) {
    StubComm* c = reinterpret_cast<StubComm*>(h);
    const size_t bytes = n * el_size(t);
    if (!c || bytes > kSlotBytes) return ncclInvalidArgument;
    memcpy(c->slots + (size_t)c->rank * kSlotBytes, s, bytes);
    if (!barrier(c)) return ncclSystemError;  // every rank has deposited its buffer
    switch (t) {
        case ncclInt64: reduce_into((int64_t*)d, c->slots, c->nranks, n, op); break;
        case ncclUint64: reduce_into((uint64_t*)d, c->slots, c->nranks, n, op); break;
        case ncclUint32: reduce_into((uint32_t*)d, c->slots, c->nranks, n, op); break;
        default: reduce_into((int32_t*)d, c->slots, c->nranks, n, op); break;
    }
    if (!barrier(c)) return ncclSystemError;  // every rank has read the slots
    return ncclSuccess;
}
// the calls inside a group complete one by one, in the same order on every rank
ncclResult_t ncclGroupStart(void) { return ncclSuccess; }
ncclResult_t ncclGroupEnd(void) { return ncclSuccess; }
const char* ncclGetErrorString(ncclResult_t) { return "stub"; }
ncclResult_t ncclGetVersion(int* v) { *v = 1; return ncclSuccess; }
}

#if MPX_STUB_ORACLE
extern "C" int orc_group_step(int N, int mode, const mpx_group_batch* b, uint32_t kv_per_group);
#endif

// ---- kernel launchers ---------------------------------------------------------------------------
// No kernel runs here, but every launcher touches memory as its kernel's contract says, so that
// engine.cpp's staging is exercised (under ASan a slot that is too small faults in here, and
// abi_driver.cpp checks what comes back):
//   * it reads every byte of every input array;
//   * an in/out array that is not state (scalars, watermarks, ret / conf_prev of the group step)
//     or that is updated in place (the proposer's groups / st / lb, the commit handler's st /
//     committed_upto) comes back with every byte inverted, which shows the copy in, the copy out
//     and the extent;
//   * it fills output k (k = 0, 1, ... over the launcher's pure outputs, in signature order) with
//     the byte 0xA0 + k over exactly the extent the kernel may write; optional outputs only
//     when given;
//   * state passed as st_in / st_out (or *_in / *_out tables) is copied across;
//   * scratch is filled over its whole stated size;
//   * values a host form reads back to size its second copy (the log encoder's rec_off, the
//     three frame encoders' dest_off, the unmarshal's result counts, the gather's *n_shorts) are
//     real values instead of a pattern.
namespace {
volatile uint64_t g_sink;
void touch(const void* p, size_t bytes) {
    uint64_t s = 0;
    for (size_t i = 0; i < bytes; ++i) s += static_cast<const uint8_t*>(p)[i];
    g_sink = g_sink + s;
}
void fill(void* p, size_t bytes, int k) {
    if (p && bytes) memset(p, 0xA0 + k, bytes);
}
void flip(void* p, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i) static_cast<uint8_t*>(p)[i] ^= 0xFF;
}
void carry(void* out, const void* in, size_t bytes) {
    touch(in, bytes);
    if (bytes && out != in) memmove(out, in, bytes);
}
void scratch(void* p, size_t bytes) {
    if (p && bytes) memset(p, 0xEE, bytes);
}
}  // namespace

namespace mpx {
hipError_t launch_accept_tally(int, const mpx_accept_reply* recs, uint64_t n,
                               const mpx_inst_state* st_in, mpx_inst_state* st_out,
                               uint64_t n_inst, int32_t, int32_t nrep, int32_t* scalars,
                               uint8_t* decided, unsigned long long*, uint32_t*, uint32_t*,
                               hipStream_t) {
    touch(recs, n * sizeof(*recs));
    carry(st_out, st_in, n_inst * sizeof(*st_in));
    flip(scalars, (1 + nrep) * sizeof(int32_t));
    fill(decided, n_inst, 0);
    return hipSuccess;
}
hipError_t launch_committed_prefix(const mpx_inst_state* st, uint64_t n_inst, int32_t,
                                   int32_t* scalars, unsigned long long*, hipStream_t) {
    touch(st, n_inst * sizeof(*st));
    flip(scalars, sizeof(int32_t));
    return hipSuccess;
}
hipError_t launch_prepare_classic(const mpx_prepare_reply* recs, uint64_t n,
                                  const mpx_prep_state* st_in, mpx_prep_state* st_out,
                                  uint64_t n_inst, int32_t, int32_t, int32_t* default_ballot,
                                  uint8_t* prepared, uint32_t*, uint32_t*, hipStream_t) {
    touch(recs, n * sizeof(*recs));
    carry(st_out, st_in, n_inst * sizeof(*st_in));
    flip(default_ballot, sizeof(int32_t));
    fill(prepared, n_inst, 0);
    return hipSuccess;
}
hipError_t launch_prepare_min(const mpx_prepare_reply_min* recs, uint64_t n,
                              const uint64_t* grp_rec_off, mpx_group_prep_state* gst,
                              uint64_t n_groups, int32_t nrep, int32_t* peer_commits,
                              mpx_prepare_effect* eff, uint32_t*, hipStream_t) {
    touch(recs, n * sizeof(*recs));
    touch(grp_rec_off, (n_groups + 1) * sizeof(uint64_t));
    touch(gst, n_groups * sizeof(*gst));
    flip(peer_commits, n_groups * nrep * sizeof(int32_t));
    fill(eff, n * sizeof(*eff), 0);
    return hipSuccess;
}
hipError_t launch_conflict_batch(const uint8_t* op, const int64_t* key, const uint64_t* inst_off,
                                 uint64_t n_inst, uint8_t* out, hipStream_t) {
    if (n_inst < 2) return hipSuccess;
    touch(inst_off, (n_inst + 1) * sizeof(uint64_t));
    touch(op, inst_off[n_inst]);
    touch(key, inst_off[n_inst] * 8);
    fill(out, n_inst - 1, 0);
    return hipSuccess;
}
#if MPX_STUB_ORACLE
bool step_one_launch_fits(int32_t, uint32_t, uint32_t) { return true; }
// the group step through the oracle; its error codes become the kernels' error-word bits
hipError_t launch_step_totals(const mpx_group_batch* b, int64_t* totals, uint32_t*, hipStream_t);
hipError_t launch_group_step(int mode, int32_t nrep, uint32_t kv_per_group, const mpx_group_batch* b,
                             uint32_t*, uint32_t* ctl, int64_t* totals, uint32_t* err,
                             hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, unsigned long long*) {
    if (ev0) hipEventRecord(ev0, s);
    // the fused form needs the per-group decided counts the oracle writes to n_decided
    std::vector<uint32_t> nd;
    mpx_group_batch bb = *b;
    if (totals && !bb.n_decided) {
        nd.resize(b->n_groups);
        bb.n_decided = nd.data();
    }
    const int rc = orc_group_step(nrep, mode, &bb, kv_per_group);
    if (rc == MPX_E_NIL_INSTANCE) *err |= kErrNil;
    else if (rc == MPX_E_BAD_ID) *err |= kErrBadId;
    else if (rc == MPX_E_KV_FULL) *err |= kErrKvFull;
    else if (rc) *err |= kErrInval;
    if (ev1) hipEventRecord(ev1, s);
    return totals ? launch_step_totals(&bb, totals, ctl, s) : hipSuccess;
}
// k_step_totals (step.hip) over host memory
hipError_t launch_step_totals(const mpx_group_batch* b, int64_t* totals, uint32_t*, hipStream_t) {
    int64_t d = 0, xi = 0, xc = 0;
    for (uint32_t g = 0; g < b->n_groups; ++g) {
        d += b->n_decided[g];
        const int64_t ei = b->executed_in[g], eo = b->executed_out[g];
        const int64_t lo = ei + 1 < 0 ? 0 : ei + 1;
        if (eo >= lo && eo < (int64_t)b->ipg) {
            const uint64_t gi0 = (uint64_t)g * b->ipg;
            xi += eo - lo + 1;
            xc += b->cmd_off[gi0 + eo + 1] - b->cmd_off[gi0 + lo];
        }
    }
    totals[0] = d;
    totals[1] = xi;
    totals[2] = xc;
    return hipSuccess;
}
#else
bool step_one_launch_fits(int32_t, uint32_t, uint32_t) { return true; }
// outputs: committed_out, executed_out, peer_out, decided, n_decided, totals (0xA0 ..); ret and
// conf_prev are in/out (the kernels leave the values of unexecuted commands)
hipError_t launch_group_step(int, int32_t nrep, uint32_t kv_per_group, const mpx_group_batch* b,
                             uint32_t* worklist, uint32_t*, int64_t* totals, uint32_t*,
                             hipStream_t, hipEvent_t, hipEvent_t, unsigned long long*) {
    const uint64_t G = b->n_groups, ni = G * b->ipg, kv = G * kv_per_group;
    if (!G) return hipSuccess;
    touch(b->grp_rec_off, (G + 1) * sizeof(uint64_t));
    touch(b->recs, b->grp_rec_off[G] * sizeof(mpx_accept_reply));
    carry(b->st_out, b->st_in, ni * sizeof(mpx_inst_state));
    touch(b->committed_in, G * 4);
    touch(b->executed_in, G * 4);
    touch(b->peer_in, G * nrep * 4);
    touch(b->cmd_off, (ni + 1) * 4);
    const uint64_t m = b->cmd_off[ni];
    touch(b->op, m);
    touch(b->key, m * 8);
    touch(b->val, m * 8);
    if (b->has_cmds) touch(b->has_cmds, ni);
    flip(b->ret, m * 8);
    if (b->conf_prev) flip(b->conf_prev, m);
    carry(b->kv_cnt_out, b->kv_cnt_in, G * 4);
    carry(b->kv_key_out, b->kv_key_in, kv * 8);
    carry(b->kv_val_out, b->kv_val_in, kv * 8);
    fill(b->committed_out, G * 4, 0);
    fill(b->executed_out, G * 4, 1);
    fill(b->peer_out, G * nrep * 4, 2);
    fill(b->decided, ni, 3);
    fill(b->n_decided, G * 4, 4);
    fill(totals, 3 * sizeof(int64_t), 5);
    touch(worklist, G * sizeof(uint32_t));  // (the engine keeps it zeroed and large enough)
    return hipSuccess;
}
hipError_t launch_step_totals(const mpx_group_batch* b, int64_t* totals, uint32_t*, hipStream_t) {
    const uint64_t G = b->n_groups;
    touch(b->n_decided, G * 4);
    touch(b->executed_in, G * 4);
    touch(b->executed_out, G * 4);
    if (G) touch(b->cmd_off, (G * b->ipg + 1) * 4);
    fill(totals, 3 * sizeof(int64_t), 0);
    return hipSuccess;
}
#endif
uint64_t apply_chunk_commands(uint64_t c, uint64_t m) { return c ? c : m; }
// the engine's pinned-staging branch for replica-sized calls (same rule as apply.hip)
bool apply_is_one_launch(const ApplyOpts& o, uint64_t m) {
    return m && m <= MPX_APPLY_SMALL_MAX && (o.path == MPX_APPLY_AUTO || o.path == MPX_APPLY_SMALL);
}
uint64_t apply_work_bytes(const KvTable&, const ApplyOpts&, uint64_t m, Carver&&) {
    return 48 * m + 256;
}
uint64_t apply_reserve_bytes(const KvTable&, const ApplyOpts&, uint64_t m) { return 48 * m + 256; }
hipError_t launch_apply(KvTable&, const uint8_t* op, const int64_t* key, const int64_t* val,
                        uint64_t m, int64_t* ret, uint8_t* conf, const ApplyOpts&, ApplyWork& w,
                        uint32_t*, hipStream_t) {
    touch(op, m);
    touch(key, m * 8);
    touch(val, m * 8);
    fill(ret, m * 8, 0);
    fill(conf, m, 1);
    scratch(w.base, w.bytes);
    return hipSuccess;
}
// the replica-batch form: nothing to compute on the stub, but the call completes (its flag)
hipError_t launch_apply_small(KvTable&, const uint8_t*, const int64_t*, const int64_t*, uint64_t,
                              int64_t*, uint8_t*, uint32_t*, hipStream_t, bool) {
    return hipSuccess;
}
hipError_t launch_kv_clear(KvTable&, hipStream_t) { return hipSuccess; }
hipError_t launch_kv_import(KvTable&, const int64_t* keys, const int64_t* vals, uint64_t n,
                            uint32_t*, hipStream_t) {
    touch(keys, n * 8);
    touch(vals, n * 8);
    return hipSuccess;
}
hipError_t launch_kv_export(KvTable&, int64_t* keys, int64_t* vals, uint64_t cap,
                            unsigned long long*, hipStream_t) {
    fill(keys, cap * 8, 0);
    fill(vals, cap * 8, 1);
    return hipSuccess;
}
uint64_t decode_work_bytes(uint64_t len, Carver&&) { return len / 8 + 256; }
hipError_t launch_decode_peer_stream(const uint8_t* buf, uint64_t len, mpx_accept_reply* ar,
                                     uint64_t ar_cap, mpx_peer_frame* oth, uint64_t oth_cap,
                                     mpx_decode_result* res, void* work, uint64_t work_bytes,
                                     hipStream_t) {
    touch(buf, len);
    fill(ar, ar_cap * sizeof(*ar), 0);
    fill(oth, oth_cap * sizeof(*oth), 1);
    fill(res, sizeof(*res), 2);  // (counts past every capacity: the host form copies the caps)
    scratch(work, work_bytes);
    return hipSuccess;
}
uint64_t stream_work_bytes(uint64_t len, Carver&&) { return len + 256; }
hipError_t launch_decode_stream(int proto, const uint8_t* buf, uint64_t len, uint64_t,
                                const StreamOuts& o, mpx_stream_result* res, void* work,
                                uint64_t work_bytes, hipStream_t) {
    touch(buf, len);
    touch(res, sizeof(*res));  // (the counts carry over from window to window)
    fill(o.ar, o.ar_cap * sizeof(*o.ar), 0);
    fill(o.prep, o.prep_cap * (proto == MPX_MODE_MIN ? sizeof(mpx_prepare_reply_min)
                                                     : sizeof(mpx_prepare_reply)), 1);
    fill(o.var, o.var_cap * sizeof(*o.var), 2);
    fill(o.oth, o.oth_cap * sizeof(*o.oth), 3);
    fill(res, sizeof(*res), 4);  // (no stop reason the host loop continues on)
    scratch(work, work_bytes);
    return hipSuccess;
}
uint64_t fanout_work_bytes(uint64_t n, Carver&&) { return 8 * n + 256; }
hipError_t launch_encode_replies(const mpx_reply_rec* recs, uint64_t n, uint32_t n_clients, uint8_t,
                                 int32_t, uint8_t* out, uint64_t* client_off, void* work,
                                 uint64_t work_bytes, uint32_t*, hipStream_t) {
    touch(recs, n * sizeof(*recs));
    fill(out, n * MPX_PROPOSE_REPLY_BYTES, 0);
    fill(client_off, ((uint64_t)n_clients + 1) * sizeof(uint64_t), 1);
    scratch(work, work_bytes);
    return hipSuccess;
}
hipError_t launch_accept_handle(int, const mpx_accept_msg* msgs, uint64_t n,
                                const mpx_acceptor_state* st_in, mpx_acceptor_state* st_out,
                                uint64_t n_inst, int32_t, const mpx_acceptor_group* groups,
                                uint64_t n_groups, uint32_t, int32_t, mpx_accept_reply* replies,
                                int32_t* reply_to, uint8_t* effect, uint32_t*, hipStream_t) {
    touch(msgs, n * sizeof(*msgs));
    carry(st_out, st_in, n_inst * sizeof(*st_in));
    touch(groups, n_groups * sizeof(*groups));
    fill(replies, n * sizeof(*replies), 0);
    fill(reply_to, n * sizeof(int32_t), 1);
    fill(effect, n, 2);
    return hipSuccess;
}
uint64_t accept_replies_work_bytes(uint64_t n, Carver&&) { return 4 * n + 256; }
// dest_off: n frames split evenly over the destinations
hipError_t launch_encode_accept_replies(int mode, const mpx_accept_reply* replies,
                                        const int32_t* reply_to, uint64_t n, uint32_t n_dest,
                                        uint8_t* out, uint64_t* dest_off, void* work,
                                        uint64_t work_bytes, uint32_t*, hipStream_t) {
    const uint64_t frame =
        mode == MPX_MODE_MIN ? MPX_ACCEPT_REPLY_FRAME_MIN : MPX_ACCEPT_REPLY_FRAME_CLASSIC;
    touch(replies, n * sizeof(*replies));
    touch(reply_to, n * sizeof(int32_t));
    for (uint64_t d = 0; d <= n_dest; ++d) dest_off[d] = n * d / n_dest * frame;
    fill(out, n * frame, 0);
    if (n) scratch(work, work_bytes);
    return hipSuccess;
}
// in place: groups, st, lb (optional); output: one slot per send_off[n_groups]
hipError_t launch_propose_handle(int, mpx_proposer_group* groups, uint64_t n_groups,
                                 const uint64_t* prop_off, const uint64_t* send_off,
                                 mpx_acceptor_state* st, mpx_inst_state* lb, uint64_t n_inst,
                                 int32_t, uint32_t, int32_t, mpx_accept_send* sends, uint32_t*,
                                 hipStream_t) {
    if (!n_groups) return hipSuccess;
    touch(prop_off, (n_groups + 1) * sizeof(uint64_t));
    touch(send_off, (n_groups + 1) * sizeof(uint64_t));
    flip(groups, n_groups * sizeof(*groups));
    flip(st, n_inst * sizeof(*st));
    if (lb) flip(lb, n_inst * sizeof(*lb));
    fill(sends, send_off[n_groups] * sizeof(*sends), 0);
    return hipSuccess;
}
// the two Accept / Commit encoders' frames: every flagged send puts one frame of `frame` bytes in
// every destination's run, so dest_off[q] = q * flagged * frame; out gets its pattern over
// dest_off[nrep] bytes, and never at or past out_cap
constexpr uint64_t kStubAcceptFrame = 24, kStubCommitFrame = MPX_COMMIT_SHORT_FRAME;
static void stub_frames(uint64_t flagged, uint64_t frame, int32_t nrep, uint8_t* out, uint64_t out_cap,
                 uint64_t* dest_off) {
    for (int32_t q = 0; q <= nrep; ++q) dest_off[q] = (uint64_t)q * flagged * frame;
    fill(out, dest_off[nrep] < out_cap ? dest_off[nrep] : out_cap, 0);
}
uint64_t accepts_work_bytes(uint32_t nrep, uint64_t n_sends, uint64_t n_inst, Carver&&) {
    return 4 * nrep * n_sends + 4 * n_inst + 256;
}
// the command arrays are read (whole) when a flagged send carries commands, the log in MIN
hipError_t launch_encode_accepts(int mode, int32_t nrep, const mpx_accept_batch* b, uint8_t* out,
                                 uint64_t out_cap, uint64_t* dest_off, void* work,
                                 uint64_t work_bytes, uint32_t*, hipStream_t) {
    const uint64_t n_inst = b->n_groups * (uint64_t)b->ipg;
    uint64_t flagged = 0;
    bool cmds = false;
    touch(b->sends, b->n_sends * sizeof(*b->sends));
    for (uint64_t i = 0; i < b->n_sends; ++i)
        if (b->sends[i].flags & MPX_PH_ACCEPT) ++flagged, cmds |= b->sends[i].n_cmds != 0;
    if (b->n_sends) touch(b->groups, b->n_groups * sizeof(*b->groups));
    if (cmds) {
        touch(b->cmd_op, b->n_cmds);
        touch(b->cmd_key, b->n_cmds * 8);
        touch(b->cmd_val, b->n_cmds * 8);
    }
    if (mode == MPX_MODE_MIN && b->n_sends) {
        touch(b->peer_commits, b->n_groups * nrep * sizeof(int32_t));
        touch(b->log_recs, n_inst * sizeof(*b->log_recs));
        touch(b->log_cmd_off, (n_inst + 1) * sizeof(uint64_t));
        touch(b->log_op, b->n_log_cmds);
        touch(b->log_key, b->n_log_cmds * 8);
        touch(b->log_val, b->n_log_cmds * 8);
    }
    stub_frames(flagged, kStubAcceptFrame, nrep, out, out_cap, dest_off);
    if (b->n_sends) scratch(work, work_bytes);
    return hipSuccess;
}
uint64_t unmarshal_work_bytes(uint64_t n_var, uint64_t n_log, Carver&&) {
    return 16 * n_var + 8 * n_log + 256;
}
// outputs in mpx_unmarshal_out's order (accepts 0xA0 .. log_val 0xAC), each over min(capacity,
// count) elements; cmd_off / log_inst_off (n_var + 1 entries) and log_cmd_off (a start per written
// log record and the end) only when given. res is real: the counts of the frames processed, and
// n_log_cmds = one command per catch-up instance, at most log_cmd_cap
hipError_t launch_unmarshal(int, const uint8_t* buf, uint64_t len, const mpx_var_frame* var,
                            uint64_t n_var, const uint64_t* d_n_var, const mpx_unmarshal_out* o,
                            mpx_unmarshal_result* res, uint64_t, void* work, uint64_t work_bytes,
                            uint32_t*, hipStream_t) {
    touch(buf, len);
    touch(var, n_var * sizeof(*var));
    mpx_unmarshal_result r{};
    r.n_var = d_n_var && *d_n_var < n_var ? *d_n_var : n_var;
    for (uint64_t i = 0; i < r.n_var; ++i) {
        r.n_accepts += var[i].code == MPX_PEER_ACCEPT;
        r.n_commits += var[i].code == MPX_PEER_COMMIT;
        r.n_cmds += var[i].n_cmds;
        r.n_log_inst += var[i].n_log;
    }
    r.n_log_cmds = std::min<uint64_t>(o->log_cmd_cap, r.n_log_inst);
    const uint64_t na = std::min<uint64_t>(o->accept_cap, r.n_accepts),
                   nc = std::min<uint64_t>(o->commit_cap, r.n_commits),
                   m = std::min<uint64_t>(o->cmd_cap, r.n_cmds),
                   li = std::min<uint64_t>(o->log_inst_cap, r.n_log_inst);
    fill(o->accepts, na * sizeof(*o->accepts), 0);
    fill(o->accept_last_committed, na * sizeof(int32_t), 1);
    fill(o->commits, nc * sizeof(*o->commits), 2);
    fill(o->cmd_off, (n_var + 1) * sizeof(uint64_t), 3);
    fill(o->op, m, 4);
    fill(o->key, m * 8, 5);
    fill(o->val, m * 8, 6);
    fill(o->log_inst_off, (n_var + 1) * sizeof(uint64_t), 7);
    fill(o->log_recs, li * sizeof(*o->log_recs), 8);
    fill(o->log_cmd_off, (li + 1) * sizeof(uint64_t), 9);
    fill(o->log_op, r.n_log_cmds, 10);
    fill(o->log_key, r.n_log_cmds * 8, 11);
    fill(o->log_val, r.n_log_cmds * 8, 12);
    *res = r;
    scratch(work, work_bytes);
    return hipSuccess;
}
// in place: st, committed_upto; outputs: effect, log_recs (optional)
hipError_t launch_commit_handle(const mpx_accept_msg* msgs, uint64_t n, mpx_acceptor_state* st,
                                uint64_t n_inst, int32_t, int32_t* committed_upto,
                                uint64_t n_groups, uint32_t, uint8_t* effect, mpx_log_rec* log_recs,
                                uint32_t*, hipStream_t) {
    touch(msgs, n * sizeof(*msgs));
    flip(st, n_inst * sizeof(*st));
    flip(committed_upto, n_groups * sizeof(int32_t));
    fill(effect, n, 0);
    fill(log_recs, n * sizeof(*log_recs), 1);
    return hipSuccess;
}
uint64_t commits_work_bytes(uint32_t nrep, uint64_t n_sends, uint64_t n_other, Carver&&) {
    return 4 * nrep * n_sends + 8 * n_other + 256;
}
hipError_t launch_encode_commits(int32_t nrep, const mpx_commit_batch* b, uint8_t* out,
                                 uint64_t out_cap, uint64_t* dest_off, void* work,
                                 uint64_t work_bytes, uint32_t*, hipStream_t) {
    uint64_t flagged = 0;
    bool cmds = false;
    touch(b->sends, b->n_sends * sizeof(*b->sends));
    for (uint64_t i = 0; i < b->n_sends; ++i)
        if (b->sends[i].flags & MPX_CS_SEND) ++flagged, cmds |= b->sends[i].n_cmds != 0;
    if (b->n_sends) touch(b->groups, b->n_groups * sizeof(*b->groups));
    if (cmds) {
        touch(b->cmd_op, b->n_cmds);
        touch(b->cmd_key, b->n_cmds * 8);
        touch(b->cmd_val, b->n_cmds * 8);
    }
    stub_frames(flagged, kStubCommitFrame, nrep, out, out_cap, dest_off);
    if (b->n_sends) scratch(work, work_bytes);
    return hipSuccess;
}
// *n_shorts: the CommitShort codes among the frames processed; msgs, count, frame_index over
// min(cap, *n_shorts) elements
hipError_t launch_gather_commit_shorts(const uint8_t* buf, uint64_t len, const mpx_peer_frame* other,
                                       uint64_t n_other, const uint64_t* d_n_other,
                                       mpx_accept_msg* msgs, int32_t* count, uint32_t* frame_index,
                                       uint64_t cap, uint64_t* n_shorts, void* work,
                                       uint64_t work_bytes, uint32_t*, hipStream_t) {
    touch(buf, len);
    touch(other, n_other * sizeof(*other));
    const uint64_t n = d_n_other && *d_n_other < n_other ? *d_n_other : n_other;
    uint64_t shorts = 0;
    for (uint64_t i = 0; i < n; ++i) shorts += other[i].code == MPX_PEER_COMMIT_SHORT;
    const uint64_t k = shorts < cap ? shorts : cap;
    fill(msgs, k * sizeof(*msgs), 0);
    fill(count, k * sizeof(int32_t), 1);
    fill(frame_index, k * sizeof(uint32_t), 2);
    *n_shorts = shorts;
    if (n_other) scratch(work, work_bytes);
    return hipSuccess;
}
uint64_t logenc_work_bytes(uint64_t n, uint64_t, Carver&&) { return 8 * n + 256; }
uint64_t logenc_max_bytes(uint64_t n, uint64_t m) { return 18 * n + 17 * m; }
// rec_off: 18 bytes per record and 17 per command, as the bound above
hipError_t launch_encode_log(int, const mpx_log_rec* recs, uint64_t n, const uint64_t* cmd_off,
                             const uint8_t* op, const int64_t* key, const int64_t* val, uint64_t m,
                             uint8_t* out, uint64_t* rec_off, void* work, uint64_t work_bytes,
                             hipStream_t) {
    touch(recs, n * sizeof(*recs));
    if (n) touch(cmd_off, (n + 1) * sizeof(uint64_t));
    touch(op, m);
    touch(key, m * 8);
    touch(val, m * 8);
    rec_off[0] = 0;
    for (uint64_t i = 1; i <= n; ++i) rec_off[i] = 18 * i + 17 * (cmd_off[i] - cmd_off[0]);
    fill(out, rec_off[n], 0);
    scratch(work, work_bytes);
    return hipSuccess;
}
// last_rec and scalars are in/out
hipError_t launch_replay_durable(const uint8_t* log, uint64_t n, int32_t inst_cap, int32_t,
                                 mpx_log_rec* recs, uint8_t* op, int64_t* key, int64_t* val,
                                 int32_t* last_rec, int32_t* scalars, uint32_t*, void* work,
                                 uint64_t work_bytes, hipStream_t) {
    touch(log, n * MPX_DURABLE_REC_BYTES);
    flip(last_rec, (uint64_t)inst_cap * sizeof(int32_t));
    flip(scalars, 2 * sizeof(int32_t));
    fill(recs, n * sizeof(*recs), 0);
    fill(op, n, 1);
    fill(key, n * 8, 2);
    fill(val, n * 8, 3);
    scratch(work, work_bytes);
    return hipSuccess;
}
uint64_t replay_work_bytes(uint64_t n, int32_t, Carver&&) { return 16 * n + 256; }
}  // namespace mpx
