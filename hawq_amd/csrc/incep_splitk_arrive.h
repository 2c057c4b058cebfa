// The arrival protocol of the split-K grouped launches (the method: incep_splitk.hip), from the K loop's end to the complete sums in the
// last arriver's registers.  A fragment, not a header, shared as text the way incep_tile_body.h is (incep_tile.h says why):
// incep_splitk.hip and incep_group_nib_splitk.hip include it once each inside their kernel, between the K loop and the epilogue, so
// both run the same stores, fences and atomic.  A workgroup that is not the last to arrive at its tile returns from the kernel here.
// It expects
//   WM, SLAB                        MFMA pixel tiles per wave (v16i acc[WM]) and int32 partial sums per slab (128 x 64)
//   gm, sm                          the workgroup's member (GroupMember) and the launch's SliceMap
//   S, z, tile                      the member's slice count, this workgroup's slice and its output tile inside the member
//   tid, lane, wave                 of the 256 threads
//   slab, counters                  the launch's workspace
//   last                            an int in LDS
    if (S > 1) {   // wave-uniform: a member's slice count
        const size_t tile_base = ((size_t)sm.slab0[gm.mi] + (size_t)tile * S) * SLAB + wave * (WM * 1024);
        int32_t *mine = slab + tile_base + (size_t)z * SLAB;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                reinterpret_cast<v4i *>(mine)[(i * 4 + q4) * 64 + lane] = v4i{acc[i][4 * q4], acc[i][4 * q4 + 1], acc[i][4 * q4 + 2], acc[i][4 * q4 + 3]};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");   // this thread's slab stores are visible chip-wide
        __syncthreads();
        int32_t *counter = counters + sm.cnt0[gm.mi] + tile;
        if (tid == 0) {
            const int arrived = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = arrived == S - 1;
        }
        __syncthreads();
        if (!last) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // every other slice's stores are visible to this workgroup
        if (tid == 0) *counter = 0;                          // all slices have arrived: nobody touches it again in this launch
        for (int j = 0; j < S; ++j) {
            if (j == z) continue;   // this workgroup's own partial is still in its registers
            const v4i *theirs = reinterpret_cast<const v4i *>(slab + tile_base + (size_t)j * SLAB);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const v4i v = theirs[(i * 4 + q4) * 64 + lane];
                    acc[i][4 * q4] += v.x, acc[i][4 * q4 + 1] += v.y, acc[i][4 * q4 + 2] += v.z, acc[i][4 * q4 + 3] += v.w;
                }
        }
    }
