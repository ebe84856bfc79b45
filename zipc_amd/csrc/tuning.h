// tuning.h -- every switch the library reads from the environment, in ONE place.
//
// None of them changes a result.  Each one stays because something outside the library sets it: most pick between two
// exact implementations of the same step, so that the suite can compare BOTH with the oracle (tests/test_gpu_fuzz.py
// runs the randomized parity loops once per setting, in a process of its own; tests/test_gpu_parity.py's VECTOR_FORMS
// holds each form to the stored deflate vectors); ZIPC_HIP_INFLATE_BLOCKS is for tools/measure_round.sh's one-wave legs; ZIPC_HIP_HOST_THREADS and ZIPC_HIP_HOST_TIMING are documented for integrators in include/zipc_hip.h.
// They are read once per process, the first time zd::tuning() is called; the defaults are what measured faster
// (DESIGN.md section 6 has the numbers).  A switch that nothing sets any more is a constant in the code that reads it.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace zd {

struct Tuning {
  // ---- deflate: which exact form of a step runs
  bool chain_peel;             // ZIPC_HIP_CHAIN=peel     hash chains by the kernel that orders equal hashes itself (lz_chain_kernel)
                               //                          instead of ordered LDS exchange (lz_chain_xchg_kernel, the default where the
                               //                          context's probe passes).  test_gpu_fuzz, test_gpu_parity "chain-peel"
  long parse_segments;         // ZIPC_HIP_PARSE_SEGMENTS  -1 (default): parse and blocks by many waves for few long streams; 0 never;
                               //                          1 whenever a stream has two segments.  test_gpu_fuzz, test_gpu_parity
  long parse_seg;              // ZIPC_HIP_PARSE_SEG       positions per parse segment (default 0: by stream length, 4096-16384).
                               //                          test_gpu_fuzz (test_long_mixed_streams_bounded), test_gpu_parity
  long match_tiles_per_group;  // ZIPC_HIP_MATCH_TILES_PER_GROUP  consecutive tiles per lz_match workgroup (default 0: by the grid).
                               //                          test_gpu_fuzz; test_gpu_match_records sets the field itself, per call
                               //                          (zipc_hip_debug_match_records), and holds every record to a serial reference
  int match_form;              // ZIPC_HIP_MATCH_FORM      0 (default): lz_match's walk chosen per tile; 1 / 2: always the first / second
                               //                          form.  test_gpu_fuzz, test_gpu_parity "match-form-1" / "match-form-2";
                               //                          test_gpu_match_records likewise: all three forms in one process
  size_t deflate_group_bytes;  // ZIPC_HIP_DEFLATE_GROUP_BYTES  source bytes per pass through the scratch (default 8 GiB; the tests: a
                               //                          few streams).  test_gpu_fuzz
  long slices, slice_min;      // ZIPC_HIP_SLICES, ZIPC_HIP_SLICE_MIN  a batch cut into slices on side queues (default 0: two slices of at
                               //                          least 2048 streams each, forms.h batch_slices; the tests force more and smaller
                               //                          ones).  test_gpu_fuzz
  // ---- inflate of one long stream by blocks (inflate.hip inflate_by_blocks, inflate_blocks.h)
  bool inflate_blocks;         // ZIPC_HIP_INFLATE_BLOCKS=0  the stream's one wave instead.  tools/measure_round.sh
  int inflate_follow;          // ZIPC_HIP_INFLATE_FOLLOW  -1 (default): sources followed inside the token run in calls of 32 MiB of
                               //                          output and more; 0 / 1 never / always.  test_gpu_fuzz
  uint64_t explore_stride;     // ZIPC_HIP_EXPLORE_STRIDE  input bytes between two explorers (default 16384: an explorer that ends on a
                               //                          false end-of-block starts again, inflate.hip).  test_gpu_fuzz
  int resolve_hops0, resolve_hops1;  // ZIPC_HIP_RESOLVE_HOPS0 / 1  links a thread follows in the first / a later resolve round
                               //                          (default 256).  test_gpu_fuzz
  // ---- host forms (many.hip many_streams; the rule of the two sub-batch settings: host_pipeline.h plan_many)
  long host_threads;           // ZIPC_HIP_HOST_THREADS    staging threads of the many-stream host forms (default 0: 8 threads or the
                               //                          core count).  include/zipc_hip.h
  long host_chunks;            // ZIPC_HIP_HOST_CHUNKS     sub-batches of those forms (default 0: 4, 6 from a GiB staged).  test_gpu_fuzz
  long host_chunk_min;         // ZIPC_HIP_HOST_CHUNK_MIN  fewest streams a sub-batch of those forms holds (default 1024).  test_gpu_fuzz
  bool host_pack;              // ZIPC_HIP_HOST_PACK=0     a sub-batch's whole destination slots come back by the copy engine instead of
                               //                          its outputs end to end by a kernel that writes the pinned memory.
                               //                          test_gpu_host_batch (test_the_copy_engine_as_the_way_back)
  bool host_timing;            // ZIPC_HIP_HOST_TIMING=1   those forms print where each sub-batch was when on stderr.  include/zipc_hip.h
};

const Tuning &tuning();  // api.hip

}  // namespace zd
