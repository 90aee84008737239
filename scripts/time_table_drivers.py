#!/usr/bin/env python3
"""A refactor of the table reductions held to the parent's own run-to-run spread:
   python scripts/time_table_drivers.py out.json PARENT1 BRANCH1 PARENT2 BRANCH2 [four more per further session]
Each of the four arguments is a directory with the `out` files of scripts/time_{clusters,representatives,linkage,dendrogram,medoids}.py
(named clusters.json .. medoids.json), run at their default sizes in the order parent, branch, parent, branch in one session.
Every list of repeats in those files becomes its median (a list of numbers as it is, a list of records by its `total_ms`), so a
script has one median per road and run -- device and host, four runs.  No threshold is fixed in advance: a branch median passes
if it lies within the parent's two medians widened by their distance, [min - spread, max + spread].  Only the device roads are
judged (the host roads time numpy and scipy); the scripts' own equality fields must all be true."""
import json
import os
import sys

import numpy as np

SCRIPTS = ("clusters", "representatives", "linkage", "dendrogram", "medoids")


def medians(node, path=""):
    """{path: median} of every list of repeats below `node`, and the equality fields met on the way"""
    found, equal = {}, {}
    if isinstance(node, dict):
        for key, value in node.items():
            at = f"{path}.{key}" if path else key
            if key.endswith("_equal"):
                equal[at] = bool(value)
            elif isinstance(value, list) and value and all(isinstance(x, dict) and "total_ms" in x for x in value):
                found[at] = float(np.median([x["total_ms"] for x in value]))
            elif isinstance(value, list) and value and all(isinstance(x, dict) for x in value):      # (time_clusters.py: clusters_ms, pairs_ms)
                for field in value[0]:
                    if field.endswith("_ms"):
                        found[f"{at}.{field}"] = float(np.median([x[field] for x in value]))
            elif isinstance(value, list) and value and key.endswith("_ms") and all(isinstance(x, (int, float)) for x in value):
                found[at] = float(np.median(value))
            elif isinstance(value, dict):
                below, same = medians(value, at)
                found.update(below), equal.update(same)
    return found, equal


def session(runs):
    """the verdict of one parent, branch, parent, branch session; a script whose four files are not all there is left out"""
    out = {"runs": list(runs), "scripts": {}, "results_equal": True, "passes": True, "not_slower": True}
    for script in SCRIPTS:
        files = [os.path.join(run, script + ".json") for run in runs]
        if not all(os.path.exists(f) for f in files):
            continue
        per_run = [medians(json.load(open(f))) for f in files]
        roads = {}
        for road in per_run[0][0]:
            parent, branch = [per_run[0][0][road], per_run[2][0][road]], [per_run[1][0][road], per_run[3][0][road]]
            entry = {"parent_median_ms": parent, "branch_median_ms": branch}
            if "host" not in road:
                spread = abs(parent[0] - parent[1])
                entry.update(parent_spread_ms=spread, allowed_ms=[min(parent) - spread, max(parent) + spread],
                             passes=all(min(parent) - spread <= b <= max(parent) + spread for b in branch),
                             not_slower=all(b <= max(parent) + spread for b in branch))
                out["passes"], out["not_slower"] = out["passes"] and entry["passes"], out["not_slower"] and entry["not_slower"]
            roads[road] = entry
        equal = all(all(run[1].values()) for run in per_run)
        out["results_equal"] = out["results_equal"] and equal
        out["scripts"][script] = {"results_equal": equal, "roads": roads}
    return out


def main():
    out_path, runs = sys.argv[1], sys.argv[2:]
    assert runs and len(runs) % 4 == 0, __doc__
    sessions = [session(runs[i:i + 4]) for i in range(0, len(runs), 4)]
    out = {"what": "the table timing scripts on the parent commit and on the branch, parent, branch, parent, branch per session: median ms "
                   "of every road and run; a device road passes if both branch medians lie within the parent's two widened by their distance",
           "results_equal": all(s["results_equal"] for s in sessions), "passes": all(s["passes"] for s in sessions),
           "not_slower": all(s["not_slower"] for s in sessions), "sessions": sessions}
    text = json.dumps(out, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
