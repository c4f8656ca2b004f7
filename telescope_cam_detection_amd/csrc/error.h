// error.h - the library's one exception type and its argument check.  No HIP here: host-only code (esrgan_host.h and the stand-alone
// checks under tools/) throws and catches the same rtd::Error as the rest of the library.
#pragma once
#include <stdexcept>
#include <string>

namespace rtd {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define RTD_CHECK(cond, code, msg)                                                     \
  do {                                                                                 \
    if (!(cond)) throw ::rtd::Error((code), std::string(msg) + " [" #cond "] at " __FILE__ ":" + std::to_string(__LINE__)); \
  } while (0)

}  // namespace rtd
