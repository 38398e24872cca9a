// wait_check.cpp -- exercises csrc/vstab_wait.h on the CPU (tests/test_wait_cpu.py builds it with ASan + UBSan and reads
// the "name value" lines it prints).  A second thread stands in for the GPU that writes the word.
#include "vstab_wait.h"

#include <cstdio>
#include <thread>

using namespace std::chrono;

static double ms_since(steady_clock::time_point t0) { return duration<double, std::milli>(steady_clock::now() - t0).count(); }

int main()
{
    {   // already at its target
        volatile unsigned word = 7;
        const auto t0 = steady_clock::now();
        const bool ok = vstab_spin_until([&] { return word == 7u; }, seconds(60));
        printf("ready_ok %d\nready_ms %.3f\n", (int)ok, ms_since(t0));
    }
    {   // set by a second thread after ~20 ms
        volatile unsigned word = 0;
        unsigned payload = 0;
        const auto t0 = steady_clock::now();
        std::thread writer([&] {
            std::this_thread::sleep_for(milliseconds(20));
            payload = 1234;
            __atomic_store_n(const_cast<unsigned*>(&word), 5u, __ATOMIC_RELEASE);
        });
        const bool ok = vstab_spin_until([&] { return vstab_seq_reached(word, 5u); }, seconds(60));
        printf("late_ok %d\nlate_ms %.3f\nlate_payload %u\n", (int)ok, ms_since(t0), ok ? payload : 0u);
        writer.join();
    }
    {   // never set: gives up once the 50 ms limit has passed
        volatile unsigned word = 0;
        const auto t0 = steady_clock::now();
        const bool ok = vstab_spin_until([&] { return word == 1u; }, milliseconds(50));
        printf("never_ok %d\nnever_ms %.3f\n", (int)ok, ms_since(t0));
    }
    printf("seq_before_wrap %d\n", (int)vstab_seq_reached(0xFFFFFFFFu, 2u));
    printf("seq_after_wrap %d\n", (int)vstab_seq_reached(2u, 0xFFFFFFFEu));
    printf("seq_equal %d\n", (int)(vstab_seq_reached(0u, 0u) && vstab_seq_reached(0xFFFFFFFFu, 0xFFFFFFFFu) && vstab_seq_reached(9u, 9u)));
    return 0;
}
