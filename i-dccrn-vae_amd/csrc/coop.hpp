// The cooperative (spin-synchronised) recurrences -- lstm_pers.hip, lstm_pers_f32.hip, lstm_coop_f32.hip, lstm_stack2_f32.hip,
// lstm_bptt_coop_f32.hip, lstm_bptt_stack2_f32.hip -- share ONE synchronisation protocol (device side, below) and ONE launch
// path with its per-device process state (host side, coop.hip).
//
// These kernels need ALL sibling workgroups resident at once (each spins on the others), so the library keeps three pieces
// of per-device process state for them (and nothing else in the library is stateful):
//   * the residency bound: workgroups a cooperative launch may use, from hipDeviceProp_t::multiProcessorCount (one workgroup
//     per CU: each launch asks for > half a CU's LDS) minus 1/16 of the CUs as head room;
//   * the launch chain: cooperative launches of different streams of one device are ordered through an event, because two
//     half-resident launches would wait for each other until the spin bound poisons both;
//   * a sticky status word in host-mapped memory: a kernel whose bounded spin ran out (outputs poisoned with NaN) also
//     stores 1 there (system scope); from then on idv_coop_last_status() and EVERY cooperative entry of the device report
//     IDV_ECOOP until idv_coop_last_status(1) acknowledges it (a sticky device error: no caller can consume it by accident).
#pragma once
#include <hip/hip_runtime.h>

#define IDV_ECOOP (-3)

// what every cooperative kernel's Args embeds.  The caller sets nrep; idv_coop_launch fills the rest.
struct CoopSync {
    unsigned* sync;           // [abort flag: 256 B][group][replica][256 B] arrive counters (word 0; from word 64, 64 words each)
    unsigned* status;         // host-mapped sticky status word or nullptr
    int nrep;                 // replicas of each arrive counter (1, 2, 4 or 8), each on a 256-byte block of its own
    int fault;                // test hook (IDV_COOP_FAULT=1): workgroup (0, 0, 0) never arrives -> the bounded spins must abort
};

// bytes in front of a launch's work buffer that hold the abort flag and the arrive counters of `groups` groups
constexpr int idv_coop_sync_bytes(int groups, int max_rep = 8) { return 256 + groups * max_rep * 256; }

// workgroups a cooperative launch may use on the current device (no device visible: the MI355X figure, 240)
extern "C" int idv_coop_max_workgroups(void);

// The one launch path: sets the kernel's dynamic-LDS attribute, zeroes the `sync_bytes` sync words in front of `work`
// (stream-ordered), fills cs->sync / status / fault (IDV_COOP_FAULT is read at every launch), takes the launch chain of the
// device, launches `kernel` (256 threads per workgroup; params[0] points at the Args that embed *cs), records the launch in
// the chain and returns the launch status.  IDV_ECOOP, with nothing launched and the status NOT consumed, while an earlier
// cooperative launch's time-out has not been acknowledged with idv_coop_last_status(1).
int idv_coop_launch_raw(const void* kernel, dim3 grid, size_t smem, hipStream_t st, void* work, size_t sync_bytes, CoopSync* cs,
                        void** params);
template <class Args>
inline int idv_coop_launch(void (*kernel)(const Args), dim3 grid, size_t smem, hipStream_t st, void* work, size_t sync_bytes, Args& a) {
    void* params[] = {&a};
    return idv_coop_launch_raw((const void*)kernel, grid, smem, st, work, sync_bytes, &a.cs, params);
}

// ---- device side ------------------------------------------------------------------------------------------------------------
constexpr unsigned long long IDV_COOP_SPIN_LIMIT_TICKS = 40000000ull;     // 0.4 s of the 100 MHz wall clock

__device__ __forceinline__ unsigned* idv_coop_abort_flag(const CoopSync& cs) { return cs.sync; }
// replica 0 of the arrive counter of `group`.  Every arriving workgroup adds to ALL replicas of its group's counter (one wave
// instruction, one lane per replica); a workgroup polls ONE replica: 1/nrep of the pollers per word, and no two groups share a
// memory channel (with the four group counters in one 16-byte block the poll round trip grew by 28 ns per polling workgroup
// of the LAUNCH: 2.8 us of a 6.2 us step at 96 workgroups)
__device__ __forceinline__ unsigned* idv_coop_counter(const CoopSync& cs, int group) {
    return cs.sync + 64 + (size_t)(group * cs.nrep) * 64;
}
// the replica that slice `sl` of a group polls
__device__ __forceinline__ unsigned* idv_coop_replica(const CoopSync& cs, unsigned* counter0, int sl) {
    return counter0 + (size_t)(sl & (cs.nrep - 1)) * 64;
}
// injected failure (tests only): true in the workgroup that has to return before its first arrive
__device__ __forceinline__ bool idv_coop_withheld(const CoopSync& cs) {
    return cs.fault && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0;
}
// whole workgroup, behind its store drain and barrier: one more arrival on every replica
__device__ __forceinline__ void idv_coop_arrive(const CoopSync& cs, unsigned* counter0, int tid) {
    if (tid < cs.nrep) __hip_atomic_fetch_add(counter0 + (size_t)tid * 64, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// thread 0 of the workgroup: wait until *counter >= want (bounded); 1 in *abort_sh when the launch is being abandoned;
// *seen (if given) <- the last value read
// (other, other_seen): a second counter read ONCE if the first check fails, i.e. only when there is time to spare
__device__ __forceinline__ void idv_coop_wait(unsigned* counter, unsigned want, unsigned* abortf, int* abort_sh, unsigned* seen = nullptr,
                                              unsigned* other = nullptr, unsigned* other_seen = nullptr) {
    const unsigned long long t0 = wall_clock64();
    unsigned long long spins = 0;
    unsigned v;
    while ((v = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < want) {
        if (other) {
            *other_seen = __hip_atomic_load(other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            other = nullptr;
        }
        __builtin_amdgcn_s_sleep(1);
        if ((++spins & 1023) == 0) {
            if (__hip_atomic_load(abortf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { *abort_sh = 1; break; }
            if (wall_clock64() - t0 > IDV_COOP_SPIN_LIMIT_TICKS) {
                __hip_atomic_store(abortf, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *abort_sh = 1;
                break;
            }
        }
    }
    if (seen) *seen = v;
}
// one thread of a workgroup that aborted
__device__ __forceinline__ void idv_coop_raise(unsigned* host_word) {
    if (host_word) __hip_atomic_store(host_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
