// The library's identity: the version of its C ABI and the words for its status codes.  Nothing here launches.
#include "../../include/ss_hotpath.h"

extern "C" int ss_abi_version(void) { return 3; }

extern "C" const char* ss_status_string(int status) {
  switch (status) {
    case SS_OK: return "ok";
    case SS_ERR_ARG: return "invalid argument";
    case SS_ERR_LAUNCH: return "kernel launch failed";
    case SS_ERR_UNSUPPORTED: return "unsupported shape";
    default: return "unknown status";
  }
}
