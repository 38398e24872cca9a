// vstab_wait.h -- the host's bounded wait on a word that a kernel writes into coherent host memory.  Nothing from HIP
// in here: tests/test_wait_cpu.py compiles it on its own.
#pragma once
#include <chrono>

// "Sequence number `have` has reached `want`", safe across the wrap-around of counters that run for a context's lifetime.
inline bool vstab_seq_reached(unsigned have, unsigned want) { return (int)(have - want) >= 0; }

// Spins until reached() is true or `limit` of wall-clock time has passed, whichever comes first, and says whether it was
// reached().  The clock is read every 1024 spins only; what the writer stored before the word is visible afterwards.
template <class Reached>
inline bool vstab_spin_until(Reached reached, std::chrono::steady_clock::duration limit)
{
    bool ok = reached();
    if (!ok) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned long spins = 1; !(ok = reached()); spins++) {
            if ((spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > limit) break;
            __builtin_ia32_pause();
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return ok;
}
