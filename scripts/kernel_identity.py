#!/usr/bin/env python3
"""kernel_identity.py <a.so> <b.so>: which gfx950 kernels differ between two builds of a library.

Prints the kernel names only in b (added), only in a (removed) and in both with different machine code
(changed), by pollnet_amd.codehash; exits 1 when any kernel changed, else 0.  A refactor that must not touch
device code builds the library before and after and runs this on the pair."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pollnet_amd.codehash import kernel_hashes  # noqa: E402


def main(a_path, b_path):
    a, b = kernel_hashes(a_path), kernel_hashes(b_path)
    added, removed = sorted(b.keys() - a.keys()), sorted(a.keys() - b.keys())
    changed = sorted(n for n in a.keys() & b.keys() if a[n] != b[n])
    for title, names in (("added", added), ("removed", removed), ("changed", changed)):
        print(f"{title}: {len(names)}")
        for n in names:
            print(f"  {n}")
    print(f"identical: {len(a.keys() & b.keys()) - len(changed)} of {len(a)} -> {len(b)} kernels")
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
