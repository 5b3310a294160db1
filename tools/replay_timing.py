"""What the latency tools of the replay entry points share (events_replay_latency.py, events_each_latency.py,
planar_events_replay_latency.py, planar_events_each_latency.py, trace_each_latency.py): the statistics of a route's
times, routes taking turns in one process, the record of a two-route comparison and the output tail. A tool keeps its
bank, its schedule, its routes and what it requires of the figures."""
import json
import subprocess

import numpy as np


def stats(us):
    a = np.asarray(us)
    return dict(n=int(a.size), median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)),
                p90_us=float(np.percentile(a, 90)), min_us=float(a.min()), max_us=float(a.max()))


def commit_of(root):
    try:
        return subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return None


def alternate(routes, once, rounds):
    """once(route) -> microseconds; the routes take turns, `rounds` times each -> {route: [microseconds]}"""
    us = {route: [] for route in routes}
    for _ in range(rounds):
        for route in routes:
            us[route].append(once(route))
    return us


def entry(name, first, second, us, **extra):
    """the record of one comparison: `extra`, the statistics of both routes, whether the second's 10th .. 90th
    percentile range lies wholly below the first's, and whether the two ranges overlap; prints its line"""
    e = dict(extra)
    f, s = e[first], e[second] = stats(us[first]), stats(us[second])
    e["second_wholly_below_first"] = bool(s["p90_us"] < f["p10_us"])
    e["ranges_overlap"] = not (s["p90_us"] < f["p10_us"] or f["p90_us"] < s["p10_us"])
    print(f"{name}: {first} {f['median_us']:8.1f} us [{f['p10_us']:.1f} .. {f['p90_us']:.1f}]   "
          f"{second} {s['median_us']:8.1f} us [{s['p10_us']:.1f} .. {s['p90_us']:.1f}]   per ranging period, "
          f"{first} / {second} = {f['median_us'] / s['median_us']:.2f}; same state: {extra.get('same_state')}",
          flush=True)
    return e


def finish(res, out, met=True):
    """writes the result to `out` if given and prints it -> the exit status: 1 if the tool's requirement is not met"""
    text = json.dumps(res, indent=1)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if met else 1
