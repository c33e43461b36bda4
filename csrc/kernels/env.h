// Environment knobs of the kernel files: one spelling of each parse. A knob is an A/B switch
// read once per process (callers keep the result in a function-local static or in a knob
// struct filled on first use), so it is set before the process starts, never inside it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace mpit {

inline bool env_set(const char* name) { return std::getenv(name) != nullptr; }

// the variable is set to exactly `value`
inline bool env_is(const char* name, const char* value) {
  const char* e = std::getenv(name);
  return e && std::strcmp(e, value) == 0;
}

// the variable is set and its text starts with '0' (an on-by-default switch turned off)
inline bool env_off(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '0';
}

// atoll of the variable (0 for text that is no number), `dflt` when unset
inline int64_t env_i64(const char* name, int64_t dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoll(e) : dflt;
}
inline int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}
// the same clamped to [lo, hi] when set (`dflt` may lie outside: "unset" stays recognisable)
inline int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::min(hi, std::atoi(e))) : dflt;
}

}  // namespace mpit
