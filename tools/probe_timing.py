"""How the probes time a call on the GPU (envmap_train_probe.py, exposure_probe.py, error_map_probe.py, dataset_rays_probe.py): device events around a batch of calls
-- a caller's view, launches and host work included -- and candidates that alternate round by round, so that a drift of the machine falls on all of them alike."""
import statistics
import sys

import torch


def timed(fn, calls, after=None):
    """microseconds per call of `calls` calls between two device events; `after`, if given, runs behind the batch, outside the time"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    if after is not None:
        after()
    return start.elapsed_time(end) * 1e3 / calls


def alternate(candidates, rounds, calls, title, after=None, warmup=None, file=sys.stdout):
    """{name: {median_us, min_us, max_us}} of {name: fn} over `rounds` rounds of `calls` calls each, behind a warm-up batch (a quarter of `calls` unless given);
    one line per candidate goes to `file`"""
    for fn in candidates.values():
        timed(fn, max(calls // 4, 1) if warmup is None else warmup, after)
    times = {name: [] for name in candidates}
    for _ in range(rounds):
        for name, fn in candidates.items():
            times[name].append(timed(fn, calls, after))
    out = {}
    for name, t in times.items():
        out[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
        print(f"{title}, {name}: median {statistics.median(t):.2f} us, min {min(t):.2f}, max {max(t):.2f} over {rounds} rounds of {calls}", file=file)
    return out
