// What a satellite unit's launch function (consensus_launch, curve_launch, curve_xlaunch, eval_launch, snap_launch,
// trans_launch) hands back to the backend, and the one check those functions make after a launch or a group of launches.
#pragma once

namespace sfl {

// code 0 (hipSuccess): every kernel was queued; else HIP's error code, with the failing launch's name in `what`
struct LaunchErr {
  const char* what = "";
  int code = 0;
  explicit operator bool() const { return code != 0; }
};

#if defined(__HIPCC__)
// after a launch or a group of launches named `what`: the error it left behind, if any (or `rc`, an error already read)
inline LaunchErr launch_err(const char* what, hipError_t rc = hipGetLastError()) { return {what, (int)rc}; }
#endif

}  // namespace sfl
