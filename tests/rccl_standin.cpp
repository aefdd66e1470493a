// A stand-in for librccl (TEST INFRASTRUCTURE, tests/test_rccl_binding.py): the entry points the library's RCCL binding
// resolves (csrc/dist.hip, Rccl::load) plus ncclCommSplit, with no GPU and no network behind them.  Built with plain
// g++ into a shared object that GPAK_RCCL_LIB points at.  What it does is set through the environment:
//   STANDIN_LOG           file that gets one line per communicator event: "init <c>", "split <parent> <c>",
//                         "split-failed <parent>", "abort <c>", "destroy <c>"
//   STANDIN_INIT_SLEEP_S  ncclCommInitRank sleeps this long first (a rendezvous that a rank is missing from)
//   STANDIN_SPLIT_FAIL    the n-th ncclCommSplit after every ncclCommInitRank fails (1 = the first)
// -DSTANDIN_NO_ABORT leaves ncclCommAbort out, as an old library would.
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <thread>

namespace {
int env_int(const char *name) { const char *v = getenv(name); return v ? atoi(v) : 0; }
void say(const char *what, long a, long b = 0) {
  const char *path = getenv("STANDIN_LOG");
  if (!path) return;
  if (FILE *f = fopen(path, "a")) {
    if (b) fprintf(f, "%s %ld %ld\n", what, a, b); else fprintf(f, "%s %ld\n", what, a);
    fclose(f);
  }
}
long n_comms = 0, n_splits = 0;
void *new_comm() { return (void *)(0x1000 + 0x10 * ++n_comms); }   // opaque to the caller, never dereferenced
}  // namespace

typedef struct { char internal[128]; } ncclUniqueId;

extern "C" {
int ncclGetUniqueId(ncclUniqueId *id) { for (char &c : id->internal) c = 7; return 0; }
int ncclCommInitRank(void **comm, int, ncclUniqueId, int) {
  if (int s = env_int("STANDIN_INIT_SLEEP_S")) std::this_thread::sleep_for(std::chrono::seconds(s));
  *comm = new_comm();
  n_splits = 0;
  say("init", (long)*comm);
  return 0;
}
int ncclCommInitAll(void **comms, int n, const int *) { for (int i = 0; i < n; i++) comms[i] = new_comm(); return 0; }
int ncclCommSplit(void *comm, int, int, void **out, void *) {
  if (++n_splits == env_int("STANDIN_SPLIT_FAIL")) { say("split-failed", (long)comm); return 1; }
  *out = new_comm();
  say("split", (long)comm, (long)*out);
  return 0;
}
#ifndef STANDIN_NO_ABORT
int ncclCommAbort(void *comm) { say("abort", (long)comm); return 0; }
#endif
int ncclCommDestroy(void *comm) { say("destroy", (long)comm); return 0; }
int ncclBroadcast(const void *, void *, size_t, int, int, void *, void *) { return 0; }
int ncclAllReduce(const void *, void *, size_t, int, int, void *, void *) { return 0; }
const char *ncclGetErrorString(int) { return "stand-in error"; }
}
