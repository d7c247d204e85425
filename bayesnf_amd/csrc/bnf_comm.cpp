// bnf_comm.cpp -- posterior gather: the RCCL all-gather behind the C ABI (include/bnf.h).  Host only: librccl is
// dlopen'ed on first use and no kernel is launched from here.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/bnf.h"
#include "bnf_host.h"

extern "C" {

namespace {
struct RcclId { char internal[BNF_COMM_ID_BYTES]; };   // ncclUniqueId (rccl.h: 128 opaque bytes)
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(RcclId*) = nullptr;
  int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*CommInitAll)(void**, int, const int*) = nullptr;     // one process, several devices (bnf_comm_create_local)
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
};
RcclApi g_rccl;
int rccl_load() {
  if (g_rccl.lib) return BNF_OK;
  // Prefer the RCCL the process has ALREADY mapped (a torch host brings its own copy under torch/lib): a second instance
  // next to it would keep its own bootstrap threads and device state.  /proc/self/maps names it; else the loader's search.
  void* lib = nullptr;
  if (FILE* mp = fopen("/proc/self/maps", "r")) {
    char line[1024];
    while (!lib && fgets(line, sizeof(line), mp)) {
      char* pth = strchr(line, '/');
      if (!pth || !strstr(pth, "librccl.so")) continue;
      pth[strcspn(pth, "\n")] = 0;
      lib = dlopen(pth, RTLD_NOW | RTLD_GLOBAL);
    }
    fclose(mp);
  }
  const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* n : names) {
    if (lib) break;
    lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  }
  if (!lib) return fail(BNF_ERR_STATE, "cannot dlopen librccl.so: %s", dlerror());
  g_rccl.GetUniqueId = (int (*)(RcclId*))dlsym(lib, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void**, int, RcclId, int))dlsym(lib, "ncclCommInitRank");
  g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(lib, "ncclAllGather");
  g_rccl.CommDestroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
  g_rccl.CommInitAll = (int (*)(void**, int, const int*))dlsym(lib, "ncclCommInitAll");
  g_rccl.GroupStart = (int (*)())dlsym(lib, "ncclGroupStart");
  g_rccl.GroupEnd = (int (*)())dlsym(lib, "ncclGroupEnd");
  // the FULL capability is decided here (bnf_comm_available), so that every rank / caller agrees up front: the
  // per-rank entry points and the one-process group forms (ncclCommInitAll / ncclGroupStart / ncclGroupEnd)
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy ||
      !g_rccl.CommInitAll || !g_rccl.GroupStart || !g_rccl.GroupEnd) {
    g_rccl = RcclApi{};
    dlclose(lib);     // (a retry opens it again: do not pile up references)
    return fail(BNF_ERR_STATE, "librccl.so lacks an expected nccl* symbol");
  }
  if (int (*get_version)(int*) = (int (*)(int*))dlsym(lib, "ncclGetVersion")) {   // NCCL API >= 2.7: ncclChar all-gather,
    int v = 0;                                                                    // group semantics as used here
    // NCCL_VERSION_CODE is major * 1000 + minor * 100 + patch up to 2.8 and major * 10000 + minor * 100 + patch from 2.9 on
    // (2.7.8 = 2708, 2.9.6 = 20906): every code below 2700 is older than 2.7 under either encoding
    if (get_version(&v) == 0 && v > 0 && v < 2700) {
      g_rccl = RcclApi{};
      dlclose(lib);
      return fail(BNF_ERR_STATE, "librccl.so reports NCCL API version %d (< 2.7)", v);
    }
  }
  g_rccl.lib = lib;
  return BNF_OK;
}
int rccl_fail(const char* what, int rc) {
  return fail(BNF_ERR_HIP, "%s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "rccl error");
}
}  // namespace

struct bnf_comm {
  void* comm = nullptr;
  int32_t world = 0, rank = 0, device = 0;
};

int bnf_comm_available(void) {   // local and cheap: dlopen + symbol resolution, no communicator id, no listener thread
  return rccl_load();
}

int bnf_comm_unique_id(void* id) {
  if (!id) return fail(BNF_ERR_INVALID, "null");
  if (int rc = rccl_load()) return rc;
  RcclId u;
  if (int rc = g_rccl.GetUniqueId(&u)) return rccl_fail("ncclGetUniqueId", rc);
  memcpy(id, u.internal, BNF_COMM_ID_BYTES);
  return BNF_OK;
}

int bnf_comm_create(const void* id, int32_t world, int32_t rank, int32_t device, bnf_comm** out) {
  if (!id || !out || world < 1 || rank < 0 || rank >= world) return fail(BNF_ERR_INVALID, "argument");
  *out = nullptr;
  if (int rc = rccl_load()) return rc;
  HIPCHK(hipSetDevice(device));
  RcclId u;
  memcpy(u.internal, id, BNF_COMM_ID_BYTES);
  bnf_comm* c = new bnf_comm();
  c->world = world; c->rank = rank; c->device = device;
  if (int rc = g_rccl.CommInitRank(&c->comm, world, u, rank)) {
    delete c;
    return rccl_fail("ncclCommInitRank", rc);
  }
  *out = c;
  return BNF_OK;
}

int bnf_allgather(bnf_comm* c, const void* send, void* recv, size_t bytes_per_rank, void* stream) {
  if (!c || !send || !recv) return fail(BNF_ERR_INVALID, "null");
  HIPCHK(hipSetDevice(c->device));
  // ncclChar = 0: byte count is dtype-agnostic
  if (int rc = g_rccl.AllGather(send, recv, bytes_per_rank, 0, c->comm, (hipStream_t)stream))
    return rccl_fail("ncclAllGather", rc);
  return BNF_OK;
}

// One process driving n devices (the reference's own shape: jax.pmap over jax.local_devices()): one communicator
// per device from ONE ncclCommInitAll -- no id, no side channel.  RCCL refuses a device listed twice.
int bnf_comm_create_local(int32_t n, const int32_t* devices, bnf_comm** out) {
  if (!devices || !out || n < 1 || n > 64) return fail(BNF_ERR_INVALID, "argument");
  for (int i = 0; i < n; ++i) out[i] = nullptr;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j)
      if (devices[i] == devices[j]) return fail(BNF_ERR_INVALID, "device %d listed twice: one RCCL rank per device", devices[i]);
  if (int rc = rccl_load()) return rc;
  int prev = 0;
  (void)hipGetDevice(&prev);
  std::vector<void*> comms((size_t)n, nullptr);
  std::vector<int> devs(devices, devices + n);
  const int rc = g_rccl.CommInitAll(comms.data(), n, devs.data());
  (void)hipSetDevice(prev);
  if (rc) return rccl_fail("ncclCommInitAll", rc);
  for (int i = 0; i < n; ++i) {
    bnf_comm* c = new bnf_comm();
    c->comm = comms[(size_t)i]; c->world = n; c->rank = i; c->device = devices[i];
    out[i] = c;
  }
  return BNF_OK;
}

// The all-gather of every local rank in ONE group call (a single host thread cannot issue them one by one: each
// would wait for its peers).  send[i] / recv[i] / stream[i] belong to comms[i]'s device.
int bnf_allgather_group(int32_t n, bnf_comm* const* comms, const void* const* send, void* const* recv,
                        size_t bytes_per_rank, void* const* streams) {
  if (!comms || !send || !recv || n < 1) return fail(BNF_ERR_INVALID, "null");
  for (int i = 0; i < n; ++i) {
    if (!comms[i] || !send[i] || !recv[i]) return fail(BNF_ERR_INVALID, "null entry %d", i);
    // the set bnf_comm_create_local made, whole and in order: a partial or permuted set would leave ranks of the
    // communicator without their call inside the group and ncclGroupEnd waiting for them
    if (comms[i]->world != n || comms[i]->rank != i)
      return fail(BNF_ERR_INVALID, "comms[%d] is rank %d of %d: the whole local set in rank order is expected (n = %d)", i,
                  comms[i]->rank, comms[i]->world, n);
    // (streams == NULL or streams[i] == NULL: that device's default stream -- a valid hipStream_t, what a torch host
    // passes for its default current stream)
  }
  if (!g_rccl.lib) return fail(BNF_ERR_STATE, "librccl.so not loaded");
  int prev = 0;
  (void)hipGetDevice(&prev);
  if (int rc = g_rccl.GroupStart()) return rccl_fail("ncclGroupStart", rc);
  int first = 0;
  for (int i = 0; i < n; ++i) {
    (void)hipSetDevice(comms[i]->device);
    const int rc = g_rccl.AllGather(send[i], recv[i], bytes_per_rank, 0, comms[i]->comm,
                                    (hipStream_t)(streams ? streams[i] : nullptr));
    if (rc && !first) first = rc;
  }
  const int rc_end = g_rccl.GroupEnd();
  (void)hipSetDevice(prev);
  if (first) return rccl_fail("ncclAllGather (group)", first);
  if (rc_end) return rccl_fail("ncclGroupEnd", rc_end);
  return BNF_OK;
}

void bnf_comm_destroy(bnf_comm* c) {
  if (!c) return;
  if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
  delete c;
}

}  // extern "C"
