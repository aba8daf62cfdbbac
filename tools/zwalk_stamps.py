#!/usr/bin/env python3
"""Diagnostic: cycles of the zero-cost frontier walk (PVT_STAMPS build, `make stamps`):
prologue (certificates + window) and walk per chain, chunks scanned per task."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pivot-scheduling_amd"), ROOT]
import torch  # noqa: E402
from pivot_place import _abi, synthetic  # noqa: E402
from pivot_place.engine import DeviceRound, PlacementEngine  # noqa: E402

H = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
lib = sys.argv[3] if len(sys.argv) > 3 else "libpivot_place_stamps.so"
MODES = {"ca_ff": _abi.PVT_CA_FF, "ca_bf": _abi.PVT_CA_BF, "vbp_ff": _abi.PVT_VBP_FF}
mode = sys.argv[4] if len(sys.argv) > 4 else "ca_bf"
eng = PlacementEngine(0, lib_path=os.path.join(ROOT, "pivot-scheduling_amd", "diag", lib))
# (slot numbers below: the slot map in pivot-scheduling_amd/csrc/pvt_stamps.h)
f = eng.lib.pvt_debug_commit_stamps
f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
CHAIN0, CHAINS = 32 + 4096, 64     # ZW_STAMP_CHAIN, ZW_STAMP_CHAINS (csrc/pvt_stamps.h)
NW = CHAIN0 + 8 * CHAINS
buf = (ctypes.c_uint64 * NW)()
assert f(eng.ctx, buf, NW) == 0
r = synthetic.make_round(MODES[mode], H, T)
dr = DeviceRound(r, eng.device)
eng.run(dr)
torch.cuda.synchronize()
assert f(eng.ctx, buf, NW) == 0
st = eng.epoch_stats()
nch = max(st["frontier_chains"] + st["list_chains"], 1)
print("%s H=%d T=%d stats=%s" % (mode, H, T, st))
print("  prologue   %10.0f cycles per chain" % (buf[0] / nch))
print("    tables + demand scan %.0f, window ids %.0f, window capacities %.0f, suffix minima %.0f"
      % tuple(buf[20 + k] / nch for k in range(4)))
# (the first phase again: up to its first barrier -- the entry loads landed and stored to LDS, the
# position map written; the fast prologue's records too -- and from there to the certificates:
# the demand scan and reductions, or the fast prologue's reductions and entry scan. With the fast
# prologue the window phases are 0: its window is part of the entry loads.)
print("    of the first phase: entry loads + position map %.0f, scan / records + reductions %.0f"
      % (buf[29] / nch, (buf[20] - buf[29]) / nch))
print("  fast-prologue chains %d" % eng.prologue_stats()["fast_chains"])
print("  walk       %10.0f cycles per chain, %.0f per task" % (buf[1] / nch, buf[1] / max(buf[3], 1)))
print("  chunks     %10.2f per task" % (buf[2] / max(buf[3], 1)))
print("  tasks      %10d, anchor switches %d" % (buf[3], buf[4]))
print("  bulk runs  %10d runs placed %d tasks (%.1f per run)" % (buf[6], buf[5], buf[5] / max(buf[6], 1)))
print("  run search %10.0f cycles per run, %.2f LDS chunk probes per run" % (buf[7] / max(buf[6], 1), buf[10] / max(buf[6], 1)))
print("  pass 1     %10.0f cycles per bulk call, %.1f iterations" % (buf[8] / max(buf[6], 1), buf[11] / max(buf[6], 1)))
print("  pass 2     %10.0f cycles per bulk call" % (buf[9] / max(buf[6], 1)))
print("    per run: setup %.0f, pass-1 loop %.0f, who loop + host ids %.0f, replay %.0f"
      % tuple(buf[24 + k] / max(buf[6], 1) for k in range(4)))
# (blocks: of ZW_UNROLL = 8 copies, the default; a variant built with another -DPVT_ZW_UNROLL reads
# wrong here. Pass 1 in copies: the loop's cycles over the copies it subtracted, block ends included; pass 2:
# "who loop + host ids" holds the host mark and the choice between snapshot and start, "replay" the
# copies after it -- a partial lane, 0 < asg < cnt, is the run's last taking lane; it replays from
# the start only where its asg lies below its snapshot)
print("    pass-1 loop: %.1f cycles per copy (%.1f copies in %.2f blocks per call)"
      % (buf[25] / max(buf[11], 1), buf[11] / max(buf[6], 1), buf[11] / 8 / max(buf[6], 1)))
print("    pass 2: snapshot choice + host ids %.0f, replay %.0f cycles per call for %.1f copies (%.1f cycles per copy)"
      % (buf[26] / max(buf[6], 1), buf[27] / max(buf[6], 1), buf[31] / max(buf[6], 1), buf[27] / max(buf[31], 1)))
print("    calls with a partial lane: %d of %d, mean asg %.1f; calls that replayed a lane from the start: %d"
      % (buf[14], buf[6], buf[15] / max(buf[14], 1), buf[30]))
print("  batches    %10.0f cycles per task (records, run masks, log flush)" % (buf[12] / max(buf[3], 1)))
print("  single     %10d tasks on the one-task hot path" % buf[13])
# per chain: run_bulk calls; those that continued a run a cap had cut (the task before the call's
# first has the same demand row, anchor and segment); the cycles from one call's return to the next
# one's entry (hot-loop re-entry, run length, batch heads: what no other stamp covers); and what the
# continued calls cost in all, each from the return before it to its own return
print("  per chain: tasks, walk cycles, run_bulk calls, continued, between-calls cycles (per call), continued calls' cycles (per call)")
for c in range(CHAINS):
    w = [int(x) for x in buf[CHAIN0 + 8 * c: CHAIN0 + 8 * c + 8]]
    if w[6] == 0:
        continue
    print("    chain %2d: %5d of %5d tasks, walk %8d, calls %4d, continued %3d, between %8d (%5.0f), continued cost %8d (%5.0f)"
          % (c, w[5], w[6], w[4], w[0], w[1], w[2], w[2] / max(w[0], 1), w[3], w[3] / max(w[1], 1)))
