/*
 * mtgpu_pipe_zones.h — ignore zones on the decode path: a pipe (mtgpu.h, "Host dispatcher") that carries a keep mask
 * (mtgpu_zones.h).  Part of the C ABI of mtgpu.h, which includes this header (include either one).  Same conventions:
 * MT_* status codes, arguments validated before anything is launched, NO CPU fallback, no environment variables.
 *
 * mtgpu_scan_zones_device tells what the trimmer WOULD keep with a mask, on a batch that is already resident.  These
 * two entry points put the mask where a recording is actually trimmed: decoder -> mtgpu_batch_add_frame ->
 * mtgpu_pipe_submit -> flags -> merge.  The keep-word layout, the rule and its consequences are those of
 * mtgpu_zones.h, with ONE plane (n_streams == 1): a pipe feeds one recording.
 *
 * Kernel (csrc/zones_kernels.hip, the pipe form): the masked scan without its stream lookup and without its clear
 * kernel — the planning kernel answers the frames without side data — and with system-scope result stores where the
 * batch's results live in pinned host memory (MT_LAYOUT_ZERO_COPY).  A submit stays planning + one kernel + one event.
 * An SD stream with a mask gets one workgroup per frame (the plain scan groups several small frames per workgroup).
 */
#ifndef MTGPU_PIPE_ZONES_H
#define MTGPU_PIPE_ZONES_H

#include "mtgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A keep mask for the decode path: the pipe (mtgpu.h, "Host dispatcher") that stands for the check_frame call in the
 * decode loop (src/motion_scanner.cpp:375-383) runs the masked scan — the active-cell test of
 * src/motion_scanner.cpp:282 ANDed with the keep bit — for every batch submitted from now on.  `keep` is ONE plane in the layout above (host memory, gh * W uint64: a pipe feeds one
 * recording, so plane 0 serves every frame); it is copied synchronously into a device plane the pipe owns, the caller's
 * buffer is free on return.  mtgpu_pipe_collect's flags are then centres >= max(1, clusters_needed) under the mask, and
 * in a pipe with MT_LAYOUT_CENTRES mtgpu_batch_centres returns the masked counts.  keep == NULL drops the mask: the
 * pipe launches the plain scan again, bit for bit as a pipe that never had one.  There is no centres_all through the
 * pipe (the staging block has no third result array): "what did the zones remove" is answered by
 * mtgpu_scan_zones_device.
 * May be called only while no batch of the pipe is being filled or in flight (states 1 and 2; batches that are
 * collected but not yet released do not matter): otherwise MT_ERR_BUSY, and nothing changes.  MT_ERR_INVALID: pipe is
 * NULL.  MT_ERR_UNSUPPORTED (the grid is named): a grid mtgpu_zones_preview rejects; the pipe keeps scanning plainly.
 * MT_ERR_DEVICE: the device cannot be selected or the copy failed.  A failing call launches nothing.  The masked scan
 * uses the batch's own work list (no launch scratch from the context's ring); with mtgpu_profile_enable on, a masked
 * submit records the same event triple as a plain one.
 */
int mtgpu_pipe_set_keep(mtgpu_pipe *pipe, const uint64_t *keep /* host, gh*W words, or NULL */);

/*
 * 1: the pipe's submits run the masked scan (src/motion_scanner.cpp:282 with the keep term, at the call site of
 * :375-383); 0: the plain scan; -1: pipe is NULL.
 */
int mtgpu_pipe_has_keep(const mtgpu_pipe *pipe);

#ifdef __cplusplus
}
#endif
#endif /* MTGPU_PIPE_ZONES_H */
