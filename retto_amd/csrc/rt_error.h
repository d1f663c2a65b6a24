// The library's exception: an RT_ERR_* code (include/retto_hip.h) and its message.  Standard library only, so the plain C++
// headers (rec_text.h) throw it too; common.h includes it for everything else.
#pragma once
#include <stdexcept>
#include <string>

namespace rt {

struct RtError : std::runtime_error {
  int code;
  RtError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

}  // namespace rt
