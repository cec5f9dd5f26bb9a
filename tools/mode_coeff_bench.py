#!/usr/bin/env python3
"""Wall time of one get_eigenmode_coefficients call against the same
sums taken on the host: a size x size full-period plane (periodic x / y, PML in z) with 50
frequencies and 18 modes (nine orders x s, p).

    device   Simulation.get_eigenmode_coefficients(monitor, [18 DiffractedPlanewave]): one
             launch over the DFT array where it lives, 18 x 50 x 8 complex sums come back
    numpy    get_flux_data (the whole DFT array crosses to the host), dft_points, the library's
             mode_table, and the eight overlap sums per (mode, frequency) in NumPy

Both are timed after one untimed call (allocation, the per-slot index arrays); medians are
reported with every sample.  max_rel_diff is the largest difference of the two paths' sums
relative to the largest sum of its (mode, frequency).

    python tools/mode_coeff_bench.py --size 256 --out profiles/modes/plane_256.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import meep_nl_amd as mp  # noqa: E402

NFREQ = 50
EX, EY, HX, HY = 0, 1, 3, 4


def numpy_sums(sim, mon, modes, res):
    """the eight sums of fields::get_overlap for a z-normal plane, from host copies"""
    f, h = sim.fields, mon.handle
    data = sim.get_flux_data(mon)
    nf = len(mon.freq)
    tab = f.mode_table(h, modes)
    pts = [f.dft_points(h, 0), f.dft_points(h, 1)]
    lists = [np.asarray(data.E).reshape(-1, nf), np.asarray(data.H).reshape(-1, nf)]
    assert np.array_equal(pts[0][:, :3], pts[1][:, :3])
    w_all = pts[0][:, 4]
    out = np.zeros((len(modes), nf, 8), dtype=complex)
    spec = [(EX, HY, 1.0, 0), (EY, HX, -1.0, 0), (HY, EX, 1.0, 1), (HX, EY, 1.0, 1)]
    for j, (c, cc, sw, which) in enumerate(spec):
        sel = pts[which][:, 3] == c
        half = np.rint(pts[which][sel, :3] * 2 * res).astype(int)
        w = w_all[sel]
        ia = np.searchsorted(tab["coords_a"], half[:, 0])
        ib = np.searchsorted(tab["coords_b"], half[:, 1])
        layer = np.searchsorted(tab["layers"], half[:, 2])
        d = lists[which][sel] / sw
        if which == 0:
            d = np.where(d != 0, d / w[:, None], d)
        for m in range(len(modes)):
            ph = tab["pa"][m, ia] * tab["pb"][m, ib]
            phase = ph[:, None] * tab["pl"][m][:, layer].T        # [point, freq]
            wc = w[:, None] * np.conj(tab["amp"][m, :, cc][None, :] * phase)
            out[m, :, j] = (wc * d).sum(0)
            out[m, :, 4 + j] = (wc * (tab["amp"][m, :, c][None, :] * phase)).sum(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-repeats", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    mp.verbosity(0)
    res = 16.0
    L = a.size / res
    cell = mp.Vector3(L, L, 2.0)
    sim = mp.Simulation(cell_size=cell, resolution=res, k_point=mp.Vector3(),
                        boundary_layers=[mp.PML(0.5, direction=mp.Z)], eps_averaging=False,
                        geometry=[mp.Block(center=mp.Vector3(0.3, -0.2, 0),
                                           size=mp.Vector3(0.4 * L, 0.3 * L, 0.25),
                                           material=mp.Medium(epsilon=4))],
                        sources=[mp.Source(mp.GaussianSource(0.5, fwidth=0.5), mp.Ex,
                                           center=mp.Vector3(0, 0, -0.5),
                                           size=mp.Vector3(L, L, 0))])
    mon = sim.add_mode_monitor(0.5, 0.4, NFREQ, mp.FluxRegion(center=mp.Vector3(0, 0, 17 / 32.0),
                                                             size=mp.Vector3(L, L, 0)))
    sim.fields.step(a.steps)
    orders = [(gx, gy, 0) for gx in (-1, 0, 1) for gy in (-1, 0, 1)]
    bands = [mp.DiffractedPlanewave(g, None, s, p) for g in orders for s, p in ((1, 0), (0, 1))]
    modes = [(b.g, b.axis, b.s, b.p) for b in bands]
    sim.get_eigenmode_coefficients(mon, bands)  # untimed: allocation, the index arrays
    dev = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        sim.get_eigenmode_coefficients(mon, bands)
        dev.append((time.perf_counter() - t0) * 1e3)
    host, rel = [], None
    if a.numpy_repeats > 0:  # (0: the device path alone)
        for _ in range(a.numpy_repeats + 1):
            t0 = time.perf_counter()
            want = numpy_sums(sim, mon, modes, res)
            host.append((time.perf_counter() - t0) * 1e3)
        host = host[1:]
        got = sim.fields.mode_coefficients(mon.handle, modes)["overlaps"]
        scale = np.abs(want).max(axis=-1, keepdims=True)
        rel = float(np.max(np.abs(got - want) / np.where(scale > 0, scale, 1.0)))
    npts = len(sim.fields.dft_points(mon.handle, 0)) + len(sim.fields.dft_points(mon.handle, 1))
    out = {"size": a.size, "nfreq": NFREQ, "modes": len(bands), "dft_points": npts,
           "dft_array_bytes": npts * NFREQ * 16,
           "device_ms_median": statistics.median(dev), "device_ms_all": dev,
           "numpy_ms_median": statistics.median(host) if host else None, "numpy_ms_all": host,
           "max_rel_diff": rel}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
