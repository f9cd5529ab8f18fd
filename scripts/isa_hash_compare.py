#!/usr/bin/env python3
"""Compare two scripts/isa_hash.py outputs kernel by kernel. path_kernel
instances are matched by their first four template parameters (MAXSUSP, COUNT,
LMODE, GEOM), so that a build which appends instance parameters (and thereby
renames every instance) can still be set against its parent: an instance of
the old build is "unchanged" when some instance of the new build with the same
four parameters has its hash.

usage: isa_hash_compare.py PARENT.json NEW.json
"""
import json
import re
import sys
from collections import defaultdict

PK = re.compile(r"path_kernelILi(\d+)ELb(\d)ELi(\d+)ELi(\d+)E((?:L[bi]n?\d+E)*)E")  # (n: a negative value)


def split(hashes):
    pk, other = defaultdict(dict), {}
    for name, h in hashes.items():
        m = PK.search(name)
        if m:
            pk[tuple(int(x) for x in m.groups()[:4])][m.group(5)] = h
        else:
            other[name] = h
    return pk, other


def main():
    old_pk, old_other = split(json.load(open(sys.argv[1])))
    new_pk, new_other = split(json.load(open(sys.argv[2])))
    changed = sorted(n for n in old_other if new_other.get(n) != old_other[n])
    added = sorted(n for n in new_other if n not in old_other)
    print(f"other kernels: {len(old_other)} in the parent, {len(changed)} changed or gone, {len(added)} added")
    for n in changed + added:
        print("  ", n)
    by_geom = defaultdict(lambda: [0, 0, 0])  # parent instances, unchanged, new instances
    for key, forms in old_pk.items():
        g = by_geom[key[3]]
        g[0] += len(forms)
        g[1] += sum(1 for h in forms.values() if h in new_pk.get(key, {}).values())
    for key, forms in new_pk.items():
        by_geom[key[3]][2] += len(forms)
    print("path_kernel instances by GEOM: parent / unchanged / new build")
    for geom in sorted(by_geom):
        print(f"  GEOM {geom}: {by_geom[geom][0]} / {by_geom[geom][1]} / {by_geom[geom][2]}")


if __name__ == "__main__":
    main()
