/*
 * wave_sync.h -- the fence between LDS accesses of the lanes of ONE wave.  Nothing else: a unit includes it without taking on any other code.
 */
#ifndef QPSK_WAVE_SYNC_H
#define QPSK_WAVE_SYNC_H

#include <hip/hip_runtime.h>

namespace qpsk {

__device__ __forceinline__ void wave_sync()      /* one wave, in-order LDS: only the compiler needs telling */
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

} // namespace qpsk

#endif
