// env.hpp -- the one reader of the KH_* environment switches ("Environment switches").  Standard C++ only: host files without a HIP
// include use it too.  Every site keeps its own `static const` (read once per process), default and clamp.
#pragma once
#include <stdlib.h>

namespace kh {
// a switch: unset or empty = `dflt`, exactly "0" = off, anything else = on
inline bool env_flag(const char* name, bool dflt) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return !(v[0] == '0' && v[1] == 0);
}
// a number (strtoll, base 0: decimal, 0x.., 0..): unset, empty or not a number = `dflt`
inline long long env_int(const char* name, long long dflt) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    char* end = nullptr;
    const long long x = strtoll(v, &end, 0);
    return end == v ? dflt : x;
}
}  // namespace kh
