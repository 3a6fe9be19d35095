#!/usr/bin/env python3
"""Host time of the one-launch streaming push alone.

    python tools/bench_push_host.py [n_streams] [pushes]

time.perf_counter around the C call kws_stream_push_i16 (through ctypes, logits asked for, product arithmetic: ONE launch), with
no synchronise inside the timed span; the stream is drained after every push, so the launch never queues behind its predecessor.
tools/bench_stream.py times push -> results complete, in which a fraction of a microsecond of host work drowns.  Prints one JSON
line: p10 / p50 / p90 in microseconds over the last three quarters of the pushes.  KWS_HIP_LIB selects another build of the
library (tools/build_variant.sh); compare builds over several processes each -- on an MI355X host a process keeps one of two
levels about 0.3 us apart from its first push to its last, whatever the build.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "keyword-spotting_amd"))
import bench
from kws import _native


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    pushes = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    ctx.load_dscnn(bench.bench_weights()[0], 12)
    ctx.stream_open(S)
    hop = torch.from_numpy(np.random.default_rng(0).integers(-3000, 3000, size=(S, 160), dtype=np.int16)).to(dev)
    logits = torch.empty((S, 12), dtype=torch.float32, device=dev)
    labels = torch.empty((S,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lib, h = ctx._lib, ctx._h
    args = (hop.data_ptr(), logits.data_ptr(), labels.data_ptr())
    lat = []
    for _ in range(pushes):
        t0 = time.perf_counter()
        rc = lib.kws_stream_push_i16(h, args[0], args[1], args[2], 0)
        t1 = time.perf_counter()
        if rc != 0:
            raise SystemExit(lib.kws_last_error(h).decode())
        lib.kws_sync(h)
        lat.append((t1 - t0) * 1e6)
    ctx.stream_close(); ctx.close()
    lat = np.array(lat[pushes // 4:])
    print(json.dumps({"library": _native.LIB_PATH, "n_streams": S, "pushes_timed": int(len(lat)),
                      "p10_us": round(float(np.percentile(lat, 10)), 3), "p50_us": round(float(np.percentile(lat, 50)), 3),
                      "p90_us": round(float(np.percentile(lat, 90)), 3)}))


if __name__ == "__main__":
    main()
