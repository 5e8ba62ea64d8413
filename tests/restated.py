"""Helpers shared by the CPU test files (a plain module, no fixtures): G1 and Fr transforms restated in plain Python
over the oracle's group law, and the parsed listing of tools/kernel_resources.py."""
import os
import re
import subprocess
import sys

from oracle import py_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g1_mul(pt, k, cv):
    k %= cv.r
    if O.is_inf(pt) or k == 0:
        return O.Z1()
    return pt if k == 1 else O.multiply(pt, k, cv)


def g1_dft(points, root, cv):
    """naive O(len^2) DFT over G1: out[k] = sum_i root^(i k) points[i]"""
    n, r = len(points), cv.r
    out = []
    for k in range(n):
        acc = O.Z1()
        for i, p in enumerate(points):
            acc = O.add(acc, g1_mul(p, pow(root, i * k % n, r), cv), cv)
        out.append(acc)
    return out


def fr_dft(vals, root, r):
    n = len(vals)
    return [sum(v * pow(root, i * k % n, r) for i, v in enumerate(vals)) % r for k in range(n)]


def kernel_resources(lib):
    """-> (tools/kernel_resources.py's listing of `lib`, its rows [(name, vgpr, agpr, sgpr, lds, scratch)])"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), lib],
                         capture_output=True, text=True, check=True).stdout
    rows = []
    for line in out.splitlines():
        m = re.match(r"(\S.*?)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            rows.append((m.group(1).strip(),) + tuple(int(m.group(i)) for i in range(2, 7)))
    return out, rows
