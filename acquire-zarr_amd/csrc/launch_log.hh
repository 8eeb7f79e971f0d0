// launch_log.hh — test seam: which kernel a launcher chose, and with what
// geometry.  Host code only; no kernel reads it.
//
// Recording is on only when $AQZ_LAUNCH_LOG=1 at first use.  A launcher asks
// launch_log_on() (one static branch when it is off) just before
// hipLaunchKernelGGL and, when on, records one line of key=value pairs.  The
// lines go into a process-wide fixed-size ring under a mutex, because
// aqz_ds_add_frame_async launches from a background thread;
// aqz_debug_launch_log (include/aqz_downsampler.h) copies and clears it.
// tests/test_gpu_launch_rules.py runs every A/B switch of the launchers
// against the oracle and reads the lines to prove each switch took effect.
#pragma once

#include <cstddef>

namespace aqz {

bool
launch_log_on();

// printf-style; a line longer than the ring's line length is truncated, and
// once the ring is full the oldest line is dropped
void
launch_log_record(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// Copies the recorded lines, oldest first, each ended by '\n', into buf (NUL
// terminated) and clears the ring.  AQZ_OK on success (an empty string when
// nothing was recorded), AQZ_INVALID_ARGUMENT when buf is null or cap is 0,
// AQZ_OVERFLOW when cap is too small for the lines held (nothing is cleared
// then).
int
launch_log_drain(char* buf, size_t cap);

} // namespace aqz
