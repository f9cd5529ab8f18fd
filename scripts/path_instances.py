#!/usr/bin/env python3
"""The path_kernel instances of a build, from a scripts/isa_hash.py output
(its keys are the device functions' mangled names).

usage: path_instances.py ISA_HASH.json > profiles/path_instances.txt
One line per instance: MAXSUSP COUNT LMODE GEOM BOXIN FIXED and the mangled
name, sorted. tests/test_instance_cases_cpu.py holds the list against
tests/instance_cases.py's REACHABLE and UNREACHABLE.
"""
import json
import re
import sys

PK = re.compile(r"^_Z\w*?\d+path_kernelILi(\d+)ELb([01])ELi(\d+)ELi(\d+)ELb([01])ELi(n?\d+)EEEv")


def main():
    rows = []
    for name in json.load(open(sys.argv[1])):
        m = PK.match(name)
        if m:
            rows.append((tuple(int(g.replace("n", "-")) for g in m.groups()), name))
    for key, name in sorted(rows):
        print(" ".join(str(k) for k in key), name)


if __name__ == "__main__":
    main()
