// fake_rccl.cpp -- a stand-in for librccl, TEST INFRASTRUCTURE ONLY (tests/test_fake_rccl.py, tests/exchange_rank.py).
//
// RCCL refuses two ranks on one device, so on a one-GPU machine the multi-rank half of csrc/dbde_gather.cpp and
// csrc/dbde_scatter.cpp can never meet a peer.  This library exports the eleven entry points csrc/dbde_rccl.h resolves
// and moves the bytes between real PROCESSES through POSIX shared memory, so that 2-4 ranks on one GPU drive every branch.
// It is reached only through DBDE_HIP_RCCL_LIBRARY; it is never built by csrc/Makefile or build(), and it measures nothing.
//
// Transport: one shared-memory segment per communicator, named from the unique id, holding one single-slot mailbox per
// ordered pair of ranks.  A message is cut into chunks of at most the mailbox size; the sender waits for the slot to be
// empty, the receiver for it to be full (flow control by two counters).  Every call is host-blocking and stream-correct:
// hipStreamSynchronize(stream) first, then device -> mailbox -> device copies that have finished when the call returns.
// That is STRICTER than RCCL's stream ordering, hence valid for any caller that is correct under RCCL.  Nothing is ever
// queued on the GPU while a rank waits for a peer.
//
// Groups: ncclGroupStart / ncclGroupEnd defer the group's operations to the outermost ncclGroupEnd, where all of them
// progress together (round-robin, so no order of posting can deadlock a matching set).  A send to self pairs with the
// receive from self of the same position and is a direct device copy.  ncclAllGather and ncclBroadcast are built from
// the same operations.
//
// Waits are bounded: DBDE_FAKE_RCCL_TIMEOUT_S seconds without progress (default 60).  On expiry the call returns
// ncclSystemError and ncclGetErrorString(ncclSystemError) names the peer and the operation that never arrived -- a
// one-sided caller error in the code under test becomes a failed assertion, never a hang.
//
// Environment: DBDE_FAKE_RCCL_TIMEOUT_S (seconds, may be fractional), DBDE_FAKE_RCCL_MAILBOX (bytes per mailbox,
// default 1 MiB; every rank of a communicator must use the same), DBDE_FAKE_RCCL_HOST=1 (host mode: buffers are host
// pointers, the two HIP calls become memcpy / nothing -- lets the transport itself be tested without a GPU).
//
// Build (tests do this into a temporary directory):
//   hipcc -O1 -fPIC -shared fake_rccl.cpp -o libdbde_fake_rccl.so -Wl,-soname,libdbde_fake_rccl.so
//         -Wl,--version-script=exports.map -lrt -pthread
#include <fcntl.h>
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#define FAKE_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kVersionCode = 990077;   // NCCL_VERSION(99, 0, 77): no RCCL has it, so a test can prove which library is in use
constexpr uint64_t kMagic = 0x4c4343526b616664ull;

struct Header {
    std::atomic<uint64_t> magic;      // set by whoever maps the fresh (zero-filled) segment first
    std::atomic<uint64_t> mailbox;    // bytes per mailbox: every rank must agree
    std::atomic<uint32_t> arrived;    // ranks that have attached
    std::atomic<uint32_t> nranks;
};

struct Box {                          // rank src -> rank dst, one chunk at a time
    std::atomic<uint64_t> written;    // chunks the sender has published
    std::atomic<uint64_t> taken;      // chunks the receiver has consumed
    uint64_t bytes;                   // length of the chunk in the slot
    uint64_t pad[5];
};

struct Op {
    enum Kind { SEND, RECV, COPY } kind;
    int peer;
    const uint8_t *src;
    uint8_t *dst;
    size_t bytes, done;
    bool started;                     // (a zero-byte message is one empty chunk)
    hipStream_t stream;
    struct Comm *comm;
};

struct Comm {
    int nranks = 0, rank = 0;
    uint8_t *base = nullptr;
    size_t map_bytes = 0;
    uint64_t mailbox = 0;
    Box *box(int src, int dst) const {
        return reinterpret_cast<Box *>(base + 64 + (size_t)(src * nranks + dst) * (sizeof(Box) + mailbox));
    }
    uint8_t *slot(int src, int dst) const { return reinterpret_cast<uint8_t *>(box(src, dst)) + sizeof(Box); }
};

std::mutex g_mutex;
std::string g_error;                              // what ncclGetErrorString(ncclSystemError / ncclInvalidUsage) says
std::map<std::string, int> g_generation;          // communicators this process has made from one id (gather, then scatter)
thread_local int t_depth = 0;
thread_local std::vector<Op> t_ops;

bool host_mode() {
    static const bool on = [] { const char *e = getenv("DBDE_FAKE_RCCL_HOST"); return e && *e && strcmp(e, "0") != 0; }();
    return on;
}

double timeout_s() {
    const char *e = getenv("DBDE_FAKE_RCCL_TIMEOUT_S");
    const double v = e && *e ? atof(e) : 60.0;
    return v > 0 ? v : 60.0;
}

uint64_t mailbox_bytes() {
    const char *e = getenv("DBDE_FAKE_RCCL_MAILBOX");
    const uint64_t v = e && *e ? strtoull(e, nullptr, 10) : (1ull << 20);
    return v ? (v + 63) / 64 * 64 : (1ull << 20);
}

double now_s() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

void nap() {
    timespec t = {0, 20000};
    nanosleep(&t, nullptr);
}

ncclResult_t fail(ncclResult_t code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
ncclResult_t fail(ncclResult_t code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lock(g_mutex);
    g_error = buf;
    return code;
}

bool stream_sync(hipStream_t s) { return host_mode() || hipStreamSynchronize(s) == hipSuccess; }

bool move(void *dst, const void *src, size_t n, hipMemcpyKind kind) {
    if (!n) return true;
    if (host_mode()) { memmove(dst, src, n); return true; }
    return hipMemcpy(dst, src, n, kind) == hipSuccess;
}

size_t dtype_bytes(ncclDataType_t t) {
    switch (t) {
        case ncclInt8: case ncclUint8: return 1;
        case ncclFloat16: case ncclBfloat16: return 2;
        case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
        case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
        default: return 0;
    }
}

// One step of one operation; true when it moved something (or finished).
bool advance(Op &op, ncclResult_t &bad) {
    Comm *c = op.comm;
    if (op.kind == Op::COPY) {
        if (!move(op.dst, op.src, op.bytes, hipMemcpyDefault)) bad = fail(ncclUnhandledCudaError, "fake rccl: device copy of %zu bytes failed", op.bytes);
        op.done = op.bytes; op.started = true;
        return true;
    }
    const bool send = op.kind == Op::SEND;
    Box *b = send ? c->box(c->rank, op.peer) : c->box(op.peer, c->rank);
    uint8_t *slot = send ? c->slot(c->rank, op.peer) : c->slot(op.peer, c->rank);
    const uint64_t w = b->written.load(std::memory_order_acquire), t = b->taken.load(std::memory_order_acquire);
    const size_t left = op.bytes - op.done, chunk = left < c->mailbox ? left : (size_t)c->mailbox;
    if (send) {
        if (w != t) return false;                     // the slot is still full
        if (!move(slot, op.src + op.done, chunk, hipMemcpyDeviceToHost)) { bad = fail(ncclUnhandledCudaError, "fake rccl: copy to the mailbox failed"); return true; }
        b->bytes = chunk;
        b->written.store(w + 1, std::memory_order_release);
    } else {
        if (w == t) return false;                     // nothing has arrived
        if (b->bytes != chunk) {
            bad = fail(ncclInvalidArgument, "fake rccl: rank %d expected a piece of %zu bytes from rank %d and met one of %llu: the two ends disagree on the message",
                       c->rank, chunk, op.peer, (unsigned long long)b->bytes);
            return true;
        }
        if (!move(op.dst + op.done, slot, chunk, hipMemcpyHostToDevice)) { bad = fail(ncclUnhandledCudaError, "fake rccl: copy from the mailbox failed"); return true; }
        b->taken.store(t + 1, std::memory_order_release);
    }
    op.done += chunk;
    op.started = true;
    return true;
}

bool finished(const Op &op) { return op.started && op.done == op.bytes; }

// Runs a set of operations to completion.  Operations to one peer in one direction share a mailbox, so only the first
// unfinished one of each (peer, direction) may move; across peers and directions they progress round-robin.
ncclResult_t run(std::vector<Op> &ops) {
    // sends to self pair, position by position, with receives from self
    std::vector<size_t> self_send, self_recv;
    for (size_t i = 0; i < ops.size(); i++) {
        if (ops[i].kind == Op::COPY || ops[i].peer != ops[i].comm->rank) continue;
        (ops[i].kind == Op::SEND ? self_send : self_recv).push_back(i);
    }
    if (self_send.size() != self_recv.size())
        return fail(ncclInvalidUsage, "fake rccl: %zu sends to self and %zu receives from self in one group", self_send.size(), self_recv.size());
    for (size_t k = 0; k < self_send.size(); k++) {
        Op &s = ops[self_send[k]], &r = ops[self_recv[k]];
        if (s.bytes != r.bytes) return fail(ncclInvalidArgument, "fake rccl: send to self of %zu bytes meets a receive of %zu", s.bytes, r.bytes);
        s.kind = Op::COPY; s.dst = r.dst;
        r.kind = Op::COPY; r.bytes = 0; r.src = r.dst;      // (done by its partner)
    }
    std::vector<hipStream_t> synced;                       // every stream the group names, once, before anything moves
    for (const Op &op : ops) {
        bool had = false;
        for (hipStream_t s : synced) had = had || s == op.stream;
        if (had) continue;
        if (!stream_sync(op.stream)) return fail(ncclUnhandledCudaError, "fake rccl: hipStreamSynchronize failed");
        synced.push_back(op.stream);
    }
    const double bound = timeout_s();
    double last = now_s();
    ncclResult_t bad = ncclSuccess;
    for (;;) {
        bool open = false, moved = false;
        std::vector<uint8_t> seen;
        for (Op &op : ops) {
            if (finished(op)) continue;
            open = true;
            if (op.kind != Op::COPY) {
                const size_t key = 2 * (size_t)op.peer + (op.kind == Op::SEND ? 0 : 1);
                if (seen.size() <= key) seen.resize(key + 1, 0);
                if (seen[key]) continue;
                seen[key] = 1;
            }
            if (advance(op, bad)) moved = true;
            if (bad != ncclSuccess) return bad;
        }
        if (!open) return ncclSuccess;
        if (moved) { last = now_s(); continue; }
        if (now_s() - last > bound) {
            size_t k = 0;
            for (const Op &op : ops) {
                if (!finished(op)) {
                    return fail(ncclSystemError, "fake rccl: rank %d waited %.1f s: %s #%zu of %zu bytes %s rank %d never met its peer (%zu bytes moved)",
                                op.comm->rank, bound, op.kind == Op::SEND ? "send" : "recv", k, op.bytes,
                                op.kind == Op::SEND ? "to" : "from", op.peer, op.done);
                }
                k++;
            }
        }
        nap();
    }
}

ncclResult_t submit(std::vector<Op> &&ops) {
    if (t_depth > 0) {
        for (Op &op : ops) t_ops.push_back(op);
        return ncclSuccess;
    }
    return run(ops);
}

Op make_op(Op::Kind kind, Comm *c, int peer, const void *src, void *dst, size_t bytes, hipStream_t stream) {
    Op op;
    op.kind = kind; op.peer = peer; op.comm = c; op.bytes = bytes; op.done = 0; op.started = false; op.stream = stream;
    op.src = static_cast<const uint8_t *>(src); op.dst = static_cast<uint8_t *>(dst);
    return op;
}

}  // namespace

FAKE_API ncclResult_t ncclGetVersion(int *version) {
    if (!version) return ncclInvalidArgument;
    *version = kVersionCode;
    return ncclSuccess;
}

FAKE_API const char *ncclGetErrorString(ncclResult_t result) {
    static thread_local std::string text;
    if (result == ncclSuccess) return "no error";
    std::lock_guard<std::mutex> lock(g_mutex);
    text = g_error.empty() ? "fake rccl: error " + std::to_string((int)result) : g_error;
    return text.c_str();
}

FAKE_API ncclResult_t ncclGetUniqueId(ncclUniqueId *id) {
    if (!id) return ncclInvalidArgument;
    static std::atomic<uint32_t> counter{0};
    memset(id->internal, 0, NCCL_UNIQUE_ID_BYTES);
    uint64_t words[4] = {kMagic, (uint64_t)getpid(), 0, counter.fetch_add(1)};
    timespec t;
    clock_gettime(CLOCK_REALTIME, &t);
    words[2] = (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec;
    memcpy(id->internal, words, sizeof words);
    if (FILE *f = fopen("/dev/urandom", "rb")) {
        const size_t got = fread(id->internal + 32, 1, 16, f);
        (void)got;
        fclose(f);
    }
    return ncclSuccess;
}

FAKE_API ncclResult_t ncclCommInitRank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank) {
    if (!comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(ncclInvalidArgument, "fake rccl: bad rank %d of %d", rank, nranks);
    uint64_t magic;
    memcpy(&magic, id.internal, 8);
    if (magic != kMagic) return fail(ncclInvalidArgument, "fake rccl: the unique id was not made by this library");
    std::string hex;
    for (int i = 8; i < 48; i++) { char b[3]; snprintf(b, sizeof b, "%02x", (unsigned char)id.internal[i]); hex += b; }
    int generation;
    { std::lock_guard<std::mutex> lock(g_mutex); generation = g_generation[hex]++; }
    const std::string name = "/dbde_fake_rccl_" + hex + "_" + std::to_string(generation);
    Comm *c = new Comm;
    c->nranks = nranks; c->rank = rank; c->mailbox = mailbox_bytes();
    c->map_bytes = 64 + (size_t)nranks * nranks * (sizeof(Box) + c->mailbox);
    const int fd = shm_open(name.c_str(), O_CREAT | O_RDWR, 0600);
    if (fd < 0) { delete c; return fail(ncclSystemError, "fake rccl: shm_open(%s) failed", name.c_str()); }
    if (ftruncate(fd, (off_t)c->map_bytes) != 0) { close(fd); shm_unlink(name.c_str()); delete c; return fail(ncclSystemError, "fake rccl: ftruncate failed"); }
    void *p = mmap(nullptr, c->map_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (p == MAP_FAILED) { shm_unlink(name.c_str()); delete c; return fail(ncclSystemError, "fake rccl: mmap failed"); }
    c->base = static_cast<uint8_t *>(p);
    static_assert(sizeof(Header) <= 64 && sizeof(Box) == 64, "segment layout");
    Header *h = reinterpret_cast<Header *>(c->base);
    uint64_t zero = 0;
    h->magic.compare_exchange_strong(zero, kMagic);
    zero = 0;
    if (!h->mailbox.compare_exchange_strong(zero, c->mailbox) && zero != c->mailbox) {
        munmap(p, c->map_bytes); delete c;
        return fail(ncclInvalidArgument, "fake rccl: the ranks disagree on DBDE_FAKE_RCCL_MAILBOX");
    }
    uint32_t none = 0;
    if (!h->nranks.compare_exchange_strong(none, (uint32_t)nranks) && none != (uint32_t)nranks) {
        munmap(p, c->map_bytes); delete c;
        return fail(ncclInvalidArgument, "fake rccl: the ranks disagree on the world size");
    }
    h->arrived.fetch_add(1);
    const double bound = timeout_s(), t0 = now_s();
    while (h->arrived.load() < (uint32_t)nranks) {
        if (now_s() - t0 > bound) {
            const uint32_t got = h->arrived.load();
            shm_unlink(name.c_str());
            munmap(p, c->map_bytes); delete c;
            return fail(ncclSystemError, "fake rccl: rank %d waited %.1f s in ncclCommInitRank: %u of %d ranks arrived", rank, bound, got, nranks);
        }
        nap();
    }
    if (rank == 0) shm_unlink(name.c_str());   // everybody holds its mapping: the name is no longer needed, and nothing is left behind
    *comm = reinterpret_cast<ncclComm_t>(c);
    return ncclSuccess;
}

FAKE_API ncclResult_t ncclCommDestroy(ncclComm_t comm) {
    Comm *c = reinterpret_cast<Comm *>(comm);
    if (!c) return ncclInvalidArgument;
    munmap(c->base, c->map_bytes);
    delete c;
    return ncclSuccess;
}

FAKE_API ncclResult_t ncclGroupStart() {
    t_depth++;
    return ncclSuccess;
}

FAKE_API ncclResult_t ncclGroupEnd() {
    if (t_depth <= 0) return fail(ncclInvalidUsage, "fake rccl: ncclGroupEnd without ncclGroupStart");
    if (--t_depth > 0) return ncclSuccess;
    std::vector<Op> ops;
    ops.swap(t_ops);
    return run(ops);
}

FAKE_API ncclResult_t ncclSend(const void *sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
    Comm *c = reinterpret_cast<Comm *>(comm);
    const size_t e = dtype_bytes(datatype);
    if (!c || !e || peer < 0 || peer >= c->nranks) return fail(ncclInvalidArgument, "fake rccl: bad ncclSend");
    if (peer == c->rank && t_depth == 0) return fail(ncclInvalidUsage, "fake rccl: a send to self outside a group can never be met");
    std::vector<Op> ops{make_op(Op::SEND, c, peer, sendbuff, nullptr, count * e, stream)};
    return submit(std::move(ops));
}

FAKE_API ncclResult_t ncclRecv(void *recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
    Comm *c = reinterpret_cast<Comm *>(comm);
    const size_t e = dtype_bytes(datatype);
    if (!c || !e || peer < 0 || peer >= c->nranks) return fail(ncclInvalidArgument, "fake rccl: bad ncclRecv");
    if (peer == c->rank && t_depth == 0) return fail(ncclInvalidUsage, "fake rccl: a receive from self outside a group can never be met");
    std::vector<Op> ops{make_op(Op::RECV, c, peer, nullptr, recvbuff, count * e, stream)};
    return submit(std::move(ops));
}

FAKE_API ncclResult_t ncclAllGather(const void *sendbuff, void *recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm,
                                    hipStream_t stream) {
    Comm *c = reinterpret_cast<Comm *>(comm);
    const size_t e = dtype_bytes(datatype);
    if (!c || !e || !sendbuff || !recvbuff) return fail(ncclInvalidArgument, "fake rccl: bad ncclAllGather");
    const size_t n = sendcount * e;
    uint8_t *out = static_cast<uint8_t *>(recvbuff);
    std::vector<Op> ops;
    if (sendbuff != out + (size_t)c->rank * n) ops.push_back(make_op(Op::COPY, c, c->rank, sendbuff, out + (size_t)c->rank * n, n, stream));
    for (int r = 0; r < c->nranks; r++) {
        if (r == c->rank) continue;
        ops.push_back(make_op(Op::SEND, c, r, sendbuff, nullptr, n, stream));
        ops.push_back(make_op(Op::RECV, c, r, nullptr, out + (size_t)r * n, n, stream));
    }
    return submit(std::move(ops));
}

FAKE_API ncclResult_t ncclBroadcast(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t datatype, int root, ncclComm_t comm,
                                    hipStream_t stream) {
    Comm *c = reinterpret_cast<Comm *>(comm);
    const size_t e = dtype_bytes(datatype);
    if (!c || !e || root < 0 || root >= c->nranks || !recvbuff) return fail(ncclInvalidArgument, "fake rccl: bad ncclBroadcast");
    const size_t n = count * e;
    std::vector<Op> ops;
    if (c->rank == root) {
        if (!sendbuff) return fail(ncclInvalidArgument, "fake rccl: ncclBroadcast root without a send buffer");
        if (sendbuff != recvbuff) ops.push_back(make_op(Op::COPY, c, root, sendbuff, recvbuff, n, stream));
        for (int r = 0; r < c->nranks; r++)
            if (r != root) ops.push_back(make_op(Op::SEND, c, r, sendbuff, nullptr, n, stream));
    } else {
        ops.push_back(make_op(Op::RECV, c, root, nullptr, recvbuff, n, stream));
    }
    return submit(std::move(ops));
}
