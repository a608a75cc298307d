// hostsim (developer tool, never shipped): the seam between the simulated HIP
// stream of hostsim_hip.cpp and the host launchers of hostsim_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

namespace hostsim {

// A "kernel" on `stream`: `fn` runs when the schedule says the stream reaches
// it (eager: now; lazy: when something waits for it), after everything
// enqueued on the stream before it.
void enqueue(hipStream_t stream, std::function<void()> fn);

}  // namespace hostsim
