// knobs.h — environment knobs of libmtgpu.so.  Internal.
//
// env_int() reads the supported knobs, all listed in include/mtgpu.h, "Environment": production settings and the
// FORCE_* / INJECT_* switches the test-suite needs to reach every kernel form and error path.
#pragma once
#include <cstdlib>

namespace mtgpu {

inline int env_int(const char *name, int dflt) {
  const char *v = std::getenv(name);
  return v ? std::atoi(v) : dflt;
}

}  // namespace mtgpu
