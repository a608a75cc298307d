// hostsim (developer tool, never shipped): csrc/kbg_comm.cpp (RCCL and the
// shared-memory transport) is left out of the build, so the communicator
// entry points of include/kbgpu.h answer KBG_E_UNSUPPORTED. Only
// communicator-less sessions run on the simulated stream.
#include "../csrc/kbg_comm.hpp"

extern "C" {
kbg_status kbg_comm_unique_id(uint8_t*) { return KBG_E_UNSUPPORTED; }
kbg_status kbg_comm_init(const uint8_t*, int32_t, int32_t, int32_t, kbg_comm** out) {
  if (out) *out = nullptr;
  return KBG_E_UNSUPPORTED;
}
kbg_status kbg_comm_init_host(const char*, int32_t, int32_t, int32_t, kbg_comm** out) {
  if (out) *out = nullptr;
  return KBG_E_UNSUPPORTED;
}
void kbg_comm_destroy(kbg_comm*) {}
kbg_status kbg_comm_ranks(const kbg_comm*, int32_t*, int32_t*) { return KBG_E_UNSUPPORTED; }
int32_t kbg_comm_transport(const kbg_comm*) { return -1; }
}
