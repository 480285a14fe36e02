// How the library refuses: an Error with a code of include/p3r.h, which the C ABI hands to the caller.  Host only (no HIP),
// so that pure host headers (ntt_plan.h) can refuse as the rest of the library does.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../include/p3r.h"

namespace p3r {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] inline void fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  throw Error(code, buf);
}

}  // namespace p3r
