// vbhem_em_host.h -- the host-side pieces of the device-resident trials loop that
// vbhem_em.hip (VBHEM) and vhem_em.hip (VHEM) share: the bounded wait for the
// per-iteration word and the pool of mapped host memory.  Defined in vbhem_em.hip.
// Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace vbhem {

// Spins on the sequence word a kernel writes to mapped host memory.  The stream is
// queried now and then: a failed launch ends the wait with its error, and a stream that
// has drained without the word ends it with hipErrorUnknown -- never an endless wait.
hipError_t em_wait_flag(const int *flag, int seq, hipStream_t st);

// A block of pinned, mapped host memory from a per-device pool of blocks that only grow
// (h: host address, d: the device's address of the same bytes).
struct EmMappedBuf {
  char *h = nullptr, *d = nullptr;
  size_t bytes = 0;
};
hipError_t em_acquire_mapped_buf(size_t bytes, EmMappedBuf &m);
void em_release_mapped_buf(const EmMappedBuf &m);

}  // namespace vbhem
