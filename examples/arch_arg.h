// --arch of the example programs: the TZ_ARCH_* number as before, or the name of the reference's network module
// (net4_simhash, net5, net6_simhash, net4_lcghash, net4_ensemble, net4_rnd; "test" for TZ_ARCH_TEST).  -1 for anything else.  arch_board gives the board
// size an architecture fixes (0: --n decides), arch_has_set whether it keeps a set of seen positions (bitvec.bin).
#pragma once
#include <cstdlib>
#include <string>

#include "takzero_hip.h"

static inline int arch_from_arg(const std::string& a) {
    if (a == "net4_simhash") return TZ_ARCH_NET4_SIMHASH;
    if (a == "net5") return TZ_ARCH_NET5;
    if (a == "net6_simhash") return TZ_ARCH_NET6_SIMHASH;
    if (a == "net4_lcghash") return TZ_ARCH_NET4_LCGHASH;
    if (a == "net4_ensemble") return TZ_ARCH_NET4_ENSEMBLE;
    if (a == "net4_rnd") return TZ_ARCH_NET4_RND;
    if (a == "test") return TZ_ARCH_TEST;
    if (a.empty() || a.find_first_not_of("0123456789") != std::string::npos) return -1;
    return atoi(a.c_str());
}

static inline int arch_board(int arch) {
    return arch == TZ_ARCH_NET5 ? 5 : arch == TZ_ARCH_NET4_SIMHASH || arch == TZ_ARCH_NET4_LCGHASH || arch == TZ_ARCH_NET4_ENSEMBLE || arch == TZ_ARCH_NET4_RND ? 4 : arch == TZ_ARCH_NET6_SIMHASH ? 6 : 0;
}

static inline bool arch_has_set(int arch) {
    return arch == TZ_ARCH_NET4_SIMHASH || arch == TZ_ARCH_NET6_SIMHASH || arch == TZ_ARCH_NET4_LCGHASH;
}
