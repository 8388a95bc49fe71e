// saf_knobs.h -- every SAF_* environment variable the library reads, in one table.
//
// All of them are development or A/B settings: nothing a caller needs, none part of the ABI.  They are read PER CALL -- tests and
// tools flip them between calls inside one process, and the library keeps no setting between calls: a C entry point that needs
// them calls read_knobs() once and hands the struct down by const reference.  (SAF_CLS_PRIORITY takes effect when a device's
// first pipeline is created: the call that creates it passes its knobs.)  read_knobs() is the only place in csrc/ that reads the
// environment.  Each knob keeps the parsing rule it grew up with; the rule is written beside the field.
#pragma once
#include <stdlib.h>

namespace saf {

struct Knobs {
  // ---- which path a fusion call takes (saf_window.hip: fuse_route)
  bool window;        // SAF_WINDOW: first character '0' = every call on the per-frame pipeline (development / A-B)
  bool window_bf16;   // SAF_WINDOW_BF16: first character '0' = bf16 volumes stay on the per-frame pipeline (A-B)
  char win_form;      // SAF_WIN_FORM: its FIRST LETTER -- 'r'ows (frame-ordered row kernel), 's'ums (order-free), 'b'ricks; 0 = unset (A-B, tests)
  bool win_maps16;    // SAF_WIN_MAPS16: first character '0' = a bf16 volume keeps fp32 map images and the frame-ordered kernel (A-B)
  bool win_frames64;  // SAF_WIN_FRAMES: atoi() == 64 = windows of 64 frames; any other value is ignored (development)
  bool win_overlap;   // SAF_WIN_OVERLAP: first character '0' = the windowed path on the caller's stream alone (A-B, per-kernel timing)
  // ---- the windowed path's schedule and launches
  bool cls_tiled;        // SAF_CLS_TILED: first character '0' = the classification never reads tiled depth copies (A-B)
  bool cls_tiled_first;  // SAF_CLS_TILED: first character '2' = a call's first unit reads the tiled copies too (tests)
  bool cls_verify;       // SAF_CLS_VERIFY: first character '1' = the self-checking classification, disagreements in stats[7] (tests)
  bool cls_priority;     // SAF_CLS_PRIORITY: atoi() != 0 = the classification stream at the device's highest priority (development)
  bool win_rgbl;         // SAF_WIN_RGBL: first character '0' = rgb and labels from the frames' own images, not the packed ones (A-B)
  bool win_xcd;          // SAF_WIN_XCD: first character '0' = the row kernel's units in linear, not XCD-compact, order (A-B)
  bool win_pretiles;     // SAF_WIN_PRETILES: first character '0' = later windows' depth tiles inside the classification chain (A-B)
  bool win_clear_beside; // SAF_WIN_CLEAR_BESIDE: first character '0' = a recycled volume's clear behind the last row kernel (A-B)
  bool win_trace;        // SAF_WIN_TRACE: set to anything = the host-side timeline of a windowed call on stderr (development)
  int win_wgs;           // SAF_WIN_WGS: atoi(); > 0 = row-kernel workgroups per CU (development)
  int win_slabs;         // SAF_WIN_SLABS: atoi(), unset = 1; >= 2 = every window cut into that many slabs of x-planes (development)
  int win_w0_slabs;      // SAF_WIN_W0_SLABS: atoi(), unset = 1; the same for the first window only (development)
  // ---- the brick form (saf_brick.hip)
  bool brick_split;     // SAF_BRICK_SPLIT: first character '0' = no build kernel, the walk kernel builds every brick (A-B)
  int brick_wgs;        // SAF_BRICK_WGS: atoi(); > 0 = walk-kernel workgroups per CU (development)
  long brick_pool_cap;  // SAF_BRICK_POOL_CAP: atol(), unset = -1; >= 0 and below the pool's size = a smaller segment pool (tests: overflow list)
  // ---- the per-frame pipeline (saf_fuse.hip)
  bool pipeline;  // SAF_PIPELINE: first character '0' = sweeps and row kernels on the caller's stream (debugging, per-kernel timing)
  int fuse_grid;  // SAF_FUSE_GRID: atoi(); > 0 = workgroups of the per-frame row kernel (development)
  // ---- clears and queries (saf_misc.hip, saf_query.hip, saf_query_wide.hip)
  int clear_wgs;      // SAF_CLEAR_WGS: atoi(); > 0 = the clear kernel's workgroups per CU (development)
  bool q_split;       // SAF_Q_SPLIT: set and atoi() == 0 = the exact-fp32 MFMA scan for every shape (A-B)
  bool q_split16;     // SAF_Q_SPLIT16: set and atoi() == 0 = 16-bit volumes through the split scan's fp32 form (A-B)
  int q_threads;      // SAF_Q_THREADS: atoi() == 512 = 512 threads per workgroup, any other value = 256; unset = 0, by the tiles' size (development)
  bool wide_mfma32;   // SAF_WIDE_MFMA: atoi() == 32 = the wide scan's 32x32x16 form, query_wide2_kernel (A-B, tests)
  bool w2_safe_wait;  // SAF_W2_SAFE_WAIT: first character '1' = the wide scan's draining wait (development)
};

inline Knobs read_knobs() {
  const auto not0 = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };  // on unless it starts with '0'
  const auto is1 = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };      // off unless it starts with '1'
  const auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
  const auto nonzero = [](const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); };  // on unless it reads as 0
  Knobs k;
  k.window = not0("SAF_WINDOW");
  k.window_bf16 = not0("SAF_WINDOW_BF16");
  const char* form = getenv("SAF_WIN_FORM");
  k.win_form = form ? form[0] : 0;
  k.win_maps16 = not0("SAF_WIN_MAPS16");
  k.win_frames64 = num("SAF_WIN_FRAMES", 0) == 64;
  k.win_overlap = not0("SAF_WIN_OVERLAP");
  const char* tiled = getenv("SAF_CLS_TILED");
  k.cls_tiled = !(tiled && tiled[0] == '0');
  k.cls_tiled_first = tiled && tiled[0] == '2';
  k.cls_verify = is1("SAF_CLS_VERIFY");
  k.cls_priority = num("SAF_CLS_PRIORITY", 0) != 0;
  k.win_rgbl = not0("SAF_WIN_RGBL");
  k.win_xcd = not0("SAF_WIN_XCD");
  k.win_pretiles = not0("SAF_WIN_PRETILES");
  k.win_clear_beside = not0("SAF_WIN_CLEAR_BESIDE");
  k.win_trace = getenv("SAF_WIN_TRACE") != nullptr;
  k.win_wgs = num("SAF_WIN_WGS", 0);
  k.win_slabs = num("SAF_WIN_SLABS", 1);
  k.win_w0_slabs = num("SAF_WIN_W0_SLABS", 1);
  k.brick_split = not0("SAF_BRICK_SPLIT");
  k.brick_wgs = num("SAF_BRICK_WGS", 0);
  const char* cap = getenv("SAF_BRICK_POOL_CAP");
  k.brick_pool_cap = cap ? atol(cap) : -1;
  k.pipeline = not0("SAF_PIPELINE");
  k.fuse_grid = num("SAF_FUSE_GRID", 0);
  k.clear_wgs = num("SAF_CLEAR_WGS", 0);
  k.q_split = nonzero("SAF_Q_SPLIT");
  k.q_split16 = nonzero("SAF_Q_SPLIT16");
  const char* th = getenv("SAF_Q_THREADS");
  k.q_threads = th ? (atoi(th) == 512 ? 512 : 256) : 0;
  k.wide_mfma32 = num("SAF_WIDE_MFMA", 0) == 32;
  k.w2_safe_wait = is1("SAF_W2_SAFE_WAIT");
  return k;
}

}  // namespace saf
