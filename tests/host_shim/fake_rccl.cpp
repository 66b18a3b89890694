// fake_rccl.cpp — a stand-in for librccl that gathers on ONE device (tests/test_comm_ranks_gpu.py). libbgs opens it through
// BGS_RCCL_LIBRARY (csrc/bgs_comm.hip, rccl_api) and runs its whole N-rank seam against it with real streams, events and
// device copies: every rank of a communicator lives in one process, one bgs_ctx per rank on the same device.
//
// HIP host code only, no kernels. Nothing here blocks or spins: a collective is complete on the host the moment its root
// calls, so the ranks of one collective are driven from one thread with the ROOT LAST. What orders the bytes is the device:
//   - a non-root rank records an event on the stream it was given and posts {send pointer, count, event};
//   - the root makes its stream wait for each sender's event and copies that sender's block behind it.
// The copy of rank r's block therefore runs behind everything rank r's communicator stream held when rank r called, as
// RCCL's does. One difference stays: a sender's call is complete on ITS stream at once, not when the root has read the
// block. A test that reuses a send buffer waits for the root's ticket first.
//
// The five nccl* symbols have RCCL's signatures (types restated here: a ROCm install without the RCCL headers builds this
// file too). The fake_rccl_* queries at the end are the tests' view of what libbgs asked for.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0, ncclUnhandledCudaError = 1, ncclSystemError = 2, ncclInternalError = 3, ncclInvalidArgument = 4,
               ncclInvalidUsage = 5 } ncclResult_t;
typedef int ncclDataType_t;   // (an enum in RCCL: an int in the calling convention)
}

namespace {
// bytes of an element, by RCCL's ncclDataType_t: int8, uint8, int32, uint32, int64, uint64, half, float, double, bfloat16
const size_t TYPE_BYTES[] = {1, 1, 4, 4, 8, 8, 2, 4, 8, 2};
constexpr int TYPE_COUNT = (int)(sizeof(TYPE_BYTES) / sizeof(TYPE_BYTES[0]));

struct Post {
    bool present = false;
    const void* send = nullptr;
    size_t count = 0;
    int datatype = 0, root = 0;
    hipEvent_t event = nullptr;
};
struct Group {
    int nranks = 0;
    std::vector<ncclComm*> members;                  // by rank; null: not (or no longer) there
    std::map<uint64_t, std::vector<Post>> posts;     // collective k -> what its senders posted, by rank
};
}  // namespace

struct ncclComm {
    std::string id;
    Group* group = nullptr;
    int rank = 0;
    uint64_t completed = 0;   // successful ncclGather calls: the next one belongs to collective `completed`
    uint64_t calls = 0;       // every ncclGather call
    int last_datatype = -1, last_root = -1, last_result = -1;
    uint64_t last_count = 0;
    hipStream_t last_stream = nullptr;
};

namespace {
constexpr char MAGIC[8] = {'F', 'A', 'K', 'E', 'R', 'C', 'C', 'L'};
std::mutex g_mutex;
std::map<std::string, Group> g_groups;
uint64_t g_ids = 0;
int g_live = 0;

void drop_posts(std::vector<Post>& posts) {
    for (Post& p : posts)
        if (p.present && p.event) (void)hipEventDestroy(p.event);   // (a recorded event is released once it has completed)
}

ncclResult_t gather_locked(ncclComm* c, const void* send, void* recv, size_t count, int datatype, int root, hipStream_t stream) {
    Group& g = *c->group;
    if (datatype < 0 || datatype >= TYPE_COUNT || root < 0 || root >= g.nranks || !send) return ncclInvalidArgument;
    const size_t bytes = count * TYPE_BYTES[datatype];
    const uint64_t k = c->completed;
    auto found = g.posts.find(k);
    if (c->rank != root) {
        if (found != g.posts.end())
            for (const Post& p : found->second)
                if (p.present && (p.count != count || p.datatype != datatype || p.root != root)) return ncclInvalidArgument;
        Post p;
        p.present = true;
        p.send = send;
        p.count = count;
        p.datatype = datatype;
        p.root = root;
        if (hipEventCreateWithFlags(&p.event, hipEventDisableTiming) != hipSuccess) return ncclUnhandledCudaError;
        if (hipEventRecord(p.event, stream) != hipSuccess) {
            (void)hipEventDestroy(p.event);
            return ncclUnhandledCudaError;
        }
        std::vector<Post>& slot = g.posts[k];
        if (slot.empty()) slot.resize((size_t)g.nranks);
        slot[(size_t)c->rank] = p;
        c->completed += 1;
        return ncclSuccess;
    }
    // the root: every other rank must have posted collective k, with the root's own arguments
    if (!recv) return ncclInvalidArgument;
    if (g.nranks > 1) {
        if (found == g.posts.end()) return ncclInvalidUsage;
        for (int r = 0; r < g.nranks; ++r)
            if (r != root && !found->second[(size_t)r].present) return ncclInvalidUsage;
        for (int r = 0; r < g.nranks; ++r) {
            const Post& p = found->second[(size_t)r];
            if (r != root && (p.count != count || p.datatype != datatype || p.root != root)) return ncclInvalidArgument;
        }
    }
    for (int r = 0; r < g.nranks; ++r) {
        const void* from = send;   // (the root's own block is in order on its stream already: no event)
        if (r != root) {
            const Post& p = found->second[(size_t)r];
            if (hipStreamWaitEvent(stream, p.event, 0) != hipSuccess) return ncclUnhandledCudaError;
            from = p.send;
        }
        if (bytes && hipMemcpyAsync((char*)recv + (size_t)r * bytes, from, bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return ncclUnhandledCudaError;
    }
    if (found != g.posts.end()) {
        drop_posts(found->second);
        g.posts.erase(found);
    }
    c->completed += 1;
    return ncclSuccess;
}

ncclComm* find_locked(const void* id, int rank) {
    if (!id) return nullptr;
    auto it = g_groups.find(std::string((const char*)id, sizeof(ncclUniqueId)));
    if (it == g_groups.end() || rank < 0 || rank >= it->second.nranks) return nullptr;
    return it->second.members[(size_t)rank];
}
}  // namespace

extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId) {
    if (!uniqueId) return ncclInvalidArgument;
    std::lock_guard<std::mutex> lock(g_mutex);
    const uint64_t n = ++g_ids;
    std::memcpy(uniqueId->internal, MAGIC, sizeof(MAGIC));
    std::memcpy(uniqueId->internal + 8, &n, sizeof(n));
    for (size_t i = 16; i < sizeof(uniqueId->internal); ++i) uniqueId->internal[i] = (char)(0x5A ^ (n * 131 + i * 7));
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank) {
    if (!comm) return ncclInvalidArgument;
    *comm = nullptr;
    if (nranks < 1 || rank < 0 || rank >= nranks) return ncclInvalidArgument;
    if (std::memcmp(commId.internal, MAGIC, sizeof(MAGIC)) != 0) return ncclInvalidArgument;   // not an id of ncclGetUniqueId
    std::lock_guard<std::mutex> lock(g_mutex);
    const std::string key(commId.internal, sizeof(commId.internal));
    auto it = g_groups.find(key);
    if (it != g_groups.end()) {
        if (it->second.nranks != nranks) return ncclInvalidArgument;
        if (it->second.members[(size_t)rank]) return ncclInvalidUsage;   // the rank is taken
    } else {
        it = g_groups.emplace(key, Group()).first;
        it->second.nranks = nranks;
        it->second.members.assign((size_t)nranks, nullptr);
    }
    ncclComm* c = new ncclComm();
    c->id = key;
    c->group = &it->second;   // (std::map: the address holds while the group is in the map)
    c->rank = rank;
    it->second.members[(size_t)rank] = c;
    g_live += 1;
    *comm = c;
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
    if (!comm) return ncclInvalidArgument;
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = g_groups.find(comm->id);
    if (it == g_groups.end() || it->second.members[(size_t)comm->rank] != comm) return ncclInvalidArgument;
    Group& g = it->second;
    g.members[(size_t)comm->rank] = nullptr;
    for (auto& kv : g.posts) {   // what this rank posted and no root has taken
        Post& p = kv.second[(size_t)comm->rank];
        if (p.present && p.event) (void)hipEventDestroy(p.event);
        p = Post();
    }
    bool empty = true;
    for (ncclComm* m : g.members) empty = empty && !m;
    if (empty) g_groups.erase(it);
    delete comm;
    g_live -= 1;
    return ncclSuccess;
}

ncclResult_t ncclGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, int root, ncclComm_t comm,
                        hipStream_t stream) {
    if (!comm) return ncclInvalidArgument;
    std::lock_guard<std::mutex> lock(g_mutex);
    comm->calls += 1;
    comm->last_datatype = datatype;
    comm->last_root = root;
    comm->last_count = sendcount;
    comm->last_stream = stream;
    const ncclResult_t r = gather_locked(comm, sendbuff, recvbuff, sendcount, datatype, root, stream);
    comm->last_result = (int)r;
    return r;
}

const char* ncclGetErrorString(ncclResult_t result) {
    switch (result) {
        case ncclSuccess: return "fake rccl: no error";
        case ncclUnhandledCudaError: return "fake rccl: a HIP call failed";
        case ncclSystemError: return "fake rccl: system error";
        case ncclInternalError: return "fake rccl: internal error";
        case ncclInvalidArgument: return "fake rccl: invalid argument (or the ranks of a collective disagree)";
        case ncclInvalidUsage: return "fake rccl: invalid usage (a rank taken twice, or a root before its senders)";
        default: return "fake rccl: unknown result";
    }
}

// ---- the tests' view -------------------------------------------------------------------------------------------------
// A communicator is named by (the 128 bytes of its id, its rank): the tests hold bgs_comm handles, not ncclComm_t.
struct fake_rccl_comm_info {
    uint64_t gather_calls;       // every ncclGather call on the communicator, failed ones included
    uint64_t gathers_completed;  // the successful ones
    uint64_t last_count;         // of the last call: sendcount, datatype, root, stream and what it returned
    uint64_t last_stream;
    int32_t last_datatype, last_root, last_result, nranks;
};

int fake_rccl_live_comms(void) {
    std::lock_guard<std::mutex> lock(g_mutex);
    return g_live;
}

// 0 and *out filled, or -1 when no live communicator has that id and rank
int fake_rccl_comm_query(const void* id, int rank, fake_rccl_comm_info* out) {
    std::lock_guard<std::mutex> lock(g_mutex);
    const ncclComm* c = find_locked(id, rank);
    if (!c || !out) return -1;
    out->gather_calls = c->calls;
    out->gathers_completed = c->completed;
    out->last_count = c->last_count;
    out->last_stream = (uint64_t)(uintptr_t)c->last_stream;
    out->last_datatype = c->last_datatype;
    out->last_root = c->last_root;
    out->last_result = c->last_result;
    out->nranks = c->group->nranks;
    return 0;
}

// posts that wait for their root, over every group (0 once every collective that was started has been completed)
uint64_t fake_rccl_pending_posts(void) {
    std::lock_guard<std::mutex> lock(g_mutex);
    uint64_t n = 0;
    for (const auto& g : g_groups)
        for (const auto& kv : g.second.posts)
            for (const Post& p : kv.second) n += p.present ? 1 : 0;
    return n;
}

}  // extern "C"
