// dbde_rccl.h -- librccl, opened at run time (dlopen "librccl.so.1": in a PyTorch process that is the copy torch has
// loaded, so the process holds ONE RCCL), which keeps single-GPU users of libdbde_hip.so free of the dependency.
// A caller that wants another build of RCCL names it in the environment variable DBDE_HIP_RCCL_LIBRARY: when that is set and
// non-empty it is opened FIRST, and a file that cannot be opened or lacks one of the eleven entry points below is an error
// (rccl() returns null, Rccl::err says why) -- never a quiet fall-back to the default names.  (LD_LIBRARY_PATH cannot do
// this in a PyTorch process: "librccl.so.1" resolves by SONAME to the copy torch has already mapped.)
// Shared by the two exchange steps of the multi-GPU path: dbde_gather.cpp (encode side) and dbde_scatter.cpp (decode side).
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cstdlib>
#include <mutex>
#include <string>

namespace dbde_rccl {

struct Rccl {
    void *handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    std::string from;   // the DBDE_HIP_RCCL_LIBRARY path, when that chose the library
    std::string err;
};

inline Rccl &rccl_state() {
    static Rccl r;
    return r;
}

inline Rccl *rccl() {
    Rccl &r = rccl_state();
    static std::once_flag once;
    std::call_once(once, [&r] {
        const char *named = getenv("DBDE_HIP_RCCL_LIBRARY");
        if (named && *named) {
            r.handle = dlopen(named, RTLD_NOW | RTLD_LOCAL);
            if (!r.handle) {
                const char *why = dlerror();
                r.err = std::string("DBDE_HIP_RCCL_LIBRARY=") + named + " cannot be opened: " + (why ? why : "unknown error");
                return;
            }
            r.from = named;
        } else {
            const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
            for (const char *n : names) {
                r.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
                if (r.handle) break;
            }
            if (!r.handle) { const char *why = dlerror(); r.err = std::string("librccl not found: ") + (why ? why : "unknown error"); return; }
        }
#define DBDE_RCCL_SYM(field, name)                                             \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.handle, #name));     \
    if (!r.field) { r.err = (r.from.empty() ? std::string("librccl") : r.from) + " lacks " #name; r.handle = nullptr; return; }
        DBDE_RCCL_SYM(GetUniqueId, ncclGetUniqueId)
        DBDE_RCCL_SYM(CommInitRank, ncclCommInitRank)
        DBDE_RCCL_SYM(CommDestroy, ncclCommDestroy)
        DBDE_RCCL_SYM(AllGather, ncclAllGather)
        DBDE_RCCL_SYM(Broadcast, ncclBroadcast)
        DBDE_RCCL_SYM(Send, ncclSend)
        DBDE_RCCL_SYM(Recv, ncclRecv)
        DBDE_RCCL_SYM(GroupStart, ncclGroupStart)
        DBDE_RCCL_SYM(GroupEnd, ncclGroupEnd)
        DBDE_RCCL_SYM(GetErrorString, ncclGetErrorString)
        DBDE_RCCL_SYM(GetVersion, ncclGetVersion)
#undef DBDE_RCCL_SYM
    });
    return r.handle ? &r : nullptr;
}

// why rccl() returned null ("" while it has not, or not yet, failed)
inline const char *rccl_error() { return rccl() ? "" : rccl_state().err.c_str(); }

}  // namespace dbde_rccl
