// pgmg_stop.h — the stop rule of pgmg_solve (include/pgmg.h "Solve to a tolerance") as one pure
// host function: plain C++ over the C ABI's structs, no HIP, so it is tested without a GPU
// (tests/test_solve_cpu.py compiles this header into a small program).
#pragma once
#include <cmath>

#include "../../include/pgmg.h"

namespace pgmg {

// what the rule remembers between checks
struct StopState {
    int checks = 0;      // checks made so far
    int streak = 0;      // consecutive checks with r_i > stall_ratio * r_{i-1}
    double r0 = 0.0;     // norm at check 0 (before any cycle)
    double prev = 0.0;   // norm at the previous check
};

// 0: the options are usable; otherwise what is wrong with them
inline const char *solve_opts_error(const pgmg_solve_opts &o)
{
    if (o.cycle != PGMG_CYCLE_V && o.cycle != PGMG_CYCLE_W && o.cycle != PGMG_CYCLE_F)
        return "unknown cycle kind";
    if (o.max_cycles < 0) return "max_cycles < 0";
    if (o.check_every < 1) return "check_every < 1";
    if (o.stall_checks < 1) return "stall_checks < 1";
    if (!(o.rtol >= 0.0) || !std::isfinite(o.rtol)) return "rtol must be finite and >= 0";
    if (!(o.atol >= 0.0) || !std::isfinite(o.atol)) return "atol must be finite and >= 0";
    if (!(o.stall_ratio >= 0.0) || !std::isfinite(o.stall_ratio))
        return "stall_ratio must be finite and >= 0";
    if (o.monitor & ~(PGMG_MON_RESIDUAL | PGMG_MON_ERROR)) return "unknown monitor bits";
    return nullptr;
}

// One check: `cycles` cycles have run and the residual norm is r.  Returns a PGMG_STOP_*
// reason, or 0 with *next = the cycles to run before the next check.  In this order: a norm
// that is not finite; the target max(atol, rtol * r0); the stall streak (a check with
// r > stall_ratio * previous extends it, anything else resets it: V-cycles are not monotone
// at the start, so one bad ratio is no stall); the cycle cap.
inline int stop_check(const pgmg_solve_opts &o, StopState &st, int cycles, double r, int *next)
{
    const int i = st.checks++;
    const double prev = st.prev;
    if (i == 0) st.r0 = r;
    st.prev = r;
    *next = 0;
    if (!std::isfinite(r)) return PGMG_STOP_NONFINITE;
    const double rel = o.rtol * st.r0;
    if (r <= (o.atol > rel ? o.atol : rel)) return PGMG_STOP_CONVERGED;
    if (i >= 1 && o.stall_ratio > 0.0) {
        st.streak = r > o.stall_ratio * prev ? st.streak + 1 : 0;
        if (st.streak >= o.stall_checks) return PGMG_STOP_STALLED;
    }
    if (cycles >= o.max_cycles) return PGMG_STOP_MAX_CYCLES;
    const int left = o.max_cycles - cycles;
    *next = o.check_every < left ? o.check_every : left;
    return 0;
}

}  // namespace pgmg
