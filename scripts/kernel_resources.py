#!/usr/bin/env python3
"""Compact per-kernel register / scratch / LDS table of one .hip file, compiled as the Makefile
compiles it: python scripts/kernel_resources.py FILE.hip [extra hipcc flags]"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from stereoanywhere_amd._native import resource_usage  # noqa: E402

with tempfile.TemporaryDirectory() as tmp:
    usage = resource_usage(sys.argv[1], tmp, extra=sys.argv[2:])
for name, u in usage.items():
    n = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    print(f"v{u['vgprs']:>4} a{u['agprs']:>4} scr{u['scratch']:>4} occ{u['occupancy']:>2} "
          f"lds{u['lds']:>7}  {n[:150]}")
