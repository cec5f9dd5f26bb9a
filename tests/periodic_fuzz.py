"""A seeded random family of periodic cells (k = 0): draw(seed, ranks) makes a plain dict from
the seed alone -- it imports neither the library nor the oracle and never looks at a result --
and build(maker, cfg, R) applies it to the periodic product (R = 1) or to a metal supercell of
R replicas per periodic axis (the oracle's, or the product's own), with the helpers of
tests/periodic_cases.py.  tests/test_gpu_periodic_fuzz.py runs the seeds of SEEDS on the GPU
against the oracle's supercell; tests/test_periodic_cpu.py checks the light-cone bound of
every seed on the oracle alone and counts what the seed lists cover.

All positions are whole numbers of half pixels (A = 8 pixels per unit, a power of two), so the
replicas' coordinates and source weights are the same dyadic numbers moved by whole periods.

The generator's rules
---------------------
Cell.   One rank: seed % 10 picks the dimension and the periodic axes: the 7 non-empty subsets
        of x, y, z in 3-D, then x, y, x + y in 2-D.  Several ranks (z slabs): 3-D with x, y or
        x + y periodic and z not.  10 .. 40 cells per axis, odd and even; with three periodic
        axes 10 .. 20 (the 5-replica check on the host stays small); some seeds 65 .. 72 along
        x (two tile columns; the other axes then at most 24).  y above 28 (three tile rows) and
        z of 32 and more (several z chunks) come from the plain range.
Walls.  Per side of a non-periodic axis a PML of 2 .. 5 cells or a metal wall: one side only
        and two unequal sides are drawn.  Never along a periodic axis.  Thicknesses that leave
        fewer than 6 PML-free cells are drawn again.  The families whose E update reads
        neighbouring components (nr, upstream, aniso) get PML along one direction at most: the
        product refuses two (tests/test_gpu_periodic_fuzz.py asserts that refusal on fixed
        configurations).
Media.  One of periodic_cases.FAMILIES, or lorentz+cond, or mu+lorentz, with the values of
        periodic_cases.materials.  The block and the slab are index boxes: along a periodic
        axis either across the seam or inside, independently per axis (so across a corner of
        two periodic axes in some seeds, inside in others); along a non-periodic axis inside
        the PML-free cells.
Stack.  One axis is the stack axis: a non-periodic one where there is one, else the last.
        Along it the slab lies in the upper part and every source at least two cells below it
        (and, with metal or PML below, two cells above that), so no D source lies inside a
        polarization box.
Sources. 1 .. 3, each a point or a volume, each with its own frequency.  Point sources: any of
        the six E / H components; per periodic axis (the stack axis apart) on the seam, half a
        pixel from it, one cell from it, or anywhere.  Volume sources: per periodic axis the
        full period, sticking out of the cell on one side by 1 .. 3 cells, or strictly inside;
        or a line along one periodic axis.  Along a non-periodic axis sources keep two cells
        from the PML, except that a free draw (below) may put one E_d point source one cell
        from a wall with PML along d.
Modes.  A 3-D seed on one rank is a fusable draw (family plain or lorentz, E-component
        sources only, none inside a PML) unless seed % 10 is 2 q or 2 q + 3 modulo 7, q =
        seed // 10: two free draws per ten seeds.  Every other seed is a free draw too: its
        family goes round the seven families without a fused step (FREE_ORDER), H-component
        sources allowed.  Two free draws (seeds 0 and 3) keep plain and lorentz and get, as
        their first source, an H-component source and an E_d point source inside a PML along d:
        the two clauses of the rule below that no family decides.
        fused_expected is True exactly when: one rank, 3-D, family plain or lorentz, no
        H-component source, no E_d source in a PML along d.
Steps.  T = min((m - 2 - out) // s, 24) with m the fewest cells of a periodic axis, out the
        most cells a volume source sticks out by (its clipped copy at the supercell's wall is
        that much nearer) plus the cells the flux plane sticks out by (it reads the
        neighbouring replica that deep, averaged Yee points included), and s = 2 for nr,
        upstream and aniso, else 1; a plane across a seam is drawn only where that leaves two
        steps.  A random split of T into calls; random initial D and B.
Monitors. A dft_fields box strictly inside the cell with four components from E, H, D, B,
        and a flux plane (a line in 2-D) with a random normal that spans the full period of its
        periodic axes or sticks out across one seam; along a non-periodic axis it may begin one
        cell from the wall, so its first centred row averages the wall plane.
"""
import numpy as np

import periodic_cases as pc

A = pc.A
FREQS = [0.6, 0.8, 1.0]
FAMILIES = pc.FAMILIES + ("lorentz+cond", "mu+lorentz")
FUSABLE = ("plain", "lorentz")
UNFUSED = tuple(f for f in FAMILIES if f not in FUSABLE)
# the families of the 28 free draws of SEEDS in turn: three rounds of the unfused ones, a fourth
# of the five plain ones among them, and at the places of the first two 3-D free draws on one
# rank (seeds 0 and 3) plain and lorentz, which there get what alone keeps them unfused: an
# H-component source, and an E_d source in a PML along d
FREE_ORDER = list(UNFUSED * 3 + UNFUSED[:5])
FREE_ORDER[12:12] = list(FUSABLE)
SUBSETS = [(3, (0,)), (3, (1,)), (3, (2,)), (3, (0, 1)), (3, (0, 2)), (3, (1, 2)), (3, (0, 1, 2)),
           (2, (0,)), (2, (1,)), (2, (0, 1))]
SLAB_SUBSETS = [(0,), (1,), (0, 1)]

# the committed seed lists (tests/test_periodic_cpu.py counts what they cover)
SEEDS = {1: list(range(40)), 2: [100, 101, 102, 103], 3: [200, 201, 202, 203]}


def _ri(rng, lo, hi):
    """an integer in [lo, hi]"""
    return int(rng.integers(lo, hi + 1))


def draw(seed, ranks=1):
    rng = np.random.default_rng([seed, ranks])
    cfg = dict(seed=seed, ranks=ranks)
    if ranks == 1:
        dim, per = SUBSETS[seed % 10]
    else:
        dim, per = 3, SLAB_SUBSETS[seed % 3]
    axes = pc.axes_of(dim)
    q, r = divmod(seed, 10)
    free3 = [(2 * q) % 7, (2 * q + 3) % 7]
    fusable = ranks == 1 and dim == 3 and r not in free3
    if fusable:
        family = FUSABLE[_ri(rng, 0, 1)]
    else:  # the k-th free draw of SEEDS takes the k-th unfused family, round and round
        if ranks > 1:
            k = 20 + seed % 4 + 4 * (ranks - 2)
        else:
            k = 3 * q + (r - 7) if dim == 2 else 12 + 2 * q + free3.index(r)
        family = FREE_ORDER[k % len(FREE_ORDER)]
    clause_h = not fusable and family == "plain"      # unfused by an H-component source alone
    clause_pml = not fusable and family == "lorentz"  # ... by an E_d source in a PML along d
    reach2 = pc.reach(family) == 2
    # ---- cells
    top = 20 if len(per) == 3 else 40
    n = [_ri(rng, 10, top) if d in axes else 0 for d in range(3)]
    if len(per) < 3 and rng.random() < 0.15:
        n = [_ri(rng, 65, 72)] + [_ri(rng, 10, 24) if d in axes else 0 for d in (1, 2)]
    if ranks > 1:
        n[2] = _ri(rng, 24, 40)
    # ---- walls of the non-periodic axes: (axis, side, cells), metal where absent
    pml, pml_axes = [], 0
    th = {d: [0, 0] for d in axes}
    for d in axes:
        if d in per:
            continue
        while True:
            t = [0 if rng.random() < 0.35 else _ri(rng, 2, 5) for _ in range(2)]
            if clause_pml and not pml_axes:
                t[0] = max(t[0], 2)  # the PML that source goes into
            if n[d] - t[0] - t[1] >= 6:
                break
        if reach2 and pml_axes and (t[0] or t[1]):
            t = [0, 0]
        pml_axes += bool(t[0] or t[1])
        th[d] = t
        pml += [(d, s, t[s]) for s in range(2) if t[s]]
    # ---- the stack axis: sources below, the slab above
    nonper = [d for d in axes if d not in per]
    stack = nonper[-1] if nonper else axes[-1]
    # the PML-free cells (a periodic stack axis: one cell kept free below the seam)
    f_lo, f_hi = th[stack][0], n[stack] - th[stack][1] - (stack in per)
    base = f_lo + (2 if stack in nonper else 0)         # the sources' lowest cell
    slab_lo = _ri(rng, base + 2, f_hi - 2)
    slab_len = _ri(rng, 1, f_hi - 1 - slab_lo)
    src_top = slab_lo - 2                               # the sources' highest cell
    # ---- block and slab as index boxes (start, length) per axis
    def box(which):
        out = []
        for d in range(3):
            if d not in axes:
                out.append((0, 1))
            elif which == "slab" and d == stack:
                out.append((slab_lo, slab_len))
            elif d in per:
                if rng.random() < 0.5:  # across the seam
                    a = _ri(rng, 1, 3)
                    out.append((n[d] - a, a + _ri(rng, 1, 3)))
                else:
                    s = _ri(rng, 2, n[d] - 5)
                    out.append((s, _ri(rng, 2, n[d] - 2 - s)))
            else:
                lo, hi = th[d][0] + 1, n[d] - th[d][1] - 1
                s = _ri(rng, lo, hi - 2)
                out.append((s, _ri(rng, 2, hi - s)))
        return out
    block, slab = box("block"), box("slab")
    # ---- sources (half-pixel coordinates)
    def inner(d):
        """the half-pixel range of a source along a non-periodic axis or the stack axis"""
        if d == stack:
            return 2 * base, 2 * src_top
        return 2 * (th[d][0] + 2), 2 * (n[d] - th[d][1] - 2)
    sources, out_cells = [], 0
    for k in range(_ri(rng, 1, 3)):
        comp = _ri(rng, 0, 2) if fusable else _ri(rng, 0, 5)
        forced = k == 0 and clause_pml and ranks == 1 and dim == 3
        if k == 0 and clause_h:
            comp = _ri(rng, 3, 5)
        if forced:
            comp = pml[0][0]
        src = dict(comp=comp, freq=0.7 + 0.05 * k, width=0.7 + 0.1 * k, amp=1.0 - 0.25 * k,
                   in_pml=False)
        if rng.random() < 0.5 or forced:
            src["kind"] = "point"
            pos = [0, 0, 0]
            for d in axes:
                if d in per and d != stack:
                    how = _ri(rng, 0, 3)
                    m = 2 * n[d]
                    pos[d] = (0, (1, m - 1)[_ri(rng, 0, 1)], (2, m - 2)[_ri(rng, 0, 1)],
                              _ri(rng, 0, m - 1))[how]
                else:
                    pos[d] = _ri(rng, *inner(d))
            # a free draw: E_d one cell from a wall with PML along d (both points it touches,
            # half a pixel to either side, lie inside a PML of two cells or more)
            if not fusable and comp < 3 and comp in nonper and th[comp][0] and \
                    (rng.random() < 0.3 or forced):
                pos[comp] = 2
                src["in_pml"] = True
            src["pos"] = pos
        else:
            src["kind"] = "volume"
            lo, hi = [0, 0, 0], [0, 0, 0]
            pa = [d for d in per if d != stack]
            line = pa[_ri(rng, 0, len(pa) - 1)] if pa and rng.random() < 0.2 else None
            for d in axes:
                m = 2 * n[d]
                if d in pa and line is None:
                    how = _ri(rng, 0, 3)
                    if how == 0:    # the full period
                        lo[d], hi[d] = 0, m
                    elif how == 1:  # sticking out below
                        o = _ri(rng, 1, 3)
                        lo[d], hi[d] = -2 * o, _ri(rng, 2, m - 8)
                        out_cells = max(out_cells, o)
                    elif how == 2:  # sticking out above
                        o = _ri(rng, 1, 3)
                        lo[d], hi[d] = _ri(rng, 8, m - 2), m + 2 * o
                        out_cells = max(out_cells, o)
                    else:           # strictly inside
                        lo[d] = _ri(rng, 2, m - 6)
                        hi[d] = _ri(rng, lo[d], m - 2)
                elif d == line:
                    lo[d], hi[d] = 0, m
                elif d in pa:       # a line's fixed coordinates
                    lo[d] = hi[d] = _ri(rng, 0, m - 1)
                else:
                    a, b = inner(d)
                    lo[d] = _ri(rng, a, b)
                    hi[d] = min(b, lo[d] + (0 if rng.random() < 0.6 else _ri(rng, 1, 6)))
            src["lo"], src["hi"] = lo, hi
        sources.append(src)
    # ---- monitors
    comps = sorted(int(c) for c in rng.choice(12, size=4, replace=False))
    dlo = [_ri(rng, 4, n[d] - 2) if d in axes else 0 for d in range(3)]
    dhi = [_ri(rng, n[d] + 2, 2 * n[d] - 4) if d in axes else 0 for d in range(3)]
    normal = axes[_ri(rng, 0, len(axes) - 1)]
    flo, fhi = [0, 0, 0], [0, 0, 0]
    cross = [d for d in per if d != normal]
    cross = cross[_ri(rng, 0, len(cross) - 1)] if cross and rng.random() < 0.5 else None
    m = min(n[d] for d in per)
    if (m - 2 - out_cells - 4) // pc.reach(family) < 2:  # too few steps would be left
        cross = None
    out_src = out_cells
    for d in axes:
        mm = 2 * n[d]
        if d == normal:
            flo[d] = fhi[d] = _ri(rng, 4, mm - 4)
        elif d == cross:  # from inside the cell across the high seam, or the low one
            flo[d], fhi[d] = ((mm - _ri(rng, 4, 8), mm + _ri(rng, 2, 6)) if rng.random() < 0.5
                              else (-_ri(rng, 2, 6), _ri(rng, 4, 8)))
            o = -flo[d] if flo[d] < 0 else fhi[d] - mm
            # the centred points reach half a pixel further, the Yee points they average one more
            # a source's clipped copy and the plane may lie on the same side: the sum counts
            out_cells = out_src + (o + 3) // 2
        elif d in per:
            flo[d], fhi[d] = 0, mm
        else:
            flo[d], fhi[d] = _ri(rng, 2, n[d] - 2), _ri(rng, n[d] + 2, mm - 2)
    # ---- steps
    T = max(1, min((m - 2 - out_cells) // pc.reach(family), 24))
    cuts = sorted(set(int(c) for c in rng.integers(1, T, size=_ri(rng, 1, 3)))) if T > 1 else []
    schedule = [b - a for a, b in zip([0] + cuts, cuts + [T])]
    cfg.update(dim=dim, per=tuple(per), n=tuple(n), pml=pml, family=family, stack=stack,
               block=block, slab=slab, sources=sources, T=T, schedule=schedule,
               init_seed=1000 + seed, dft=dict(comps=comps, lo=dlo, hi=dhi),
               flux=dict(normal=normal, lo=flo, hi=fhi), fusable_draw=bool(fusable),
               out_cells=out_cells)
    cfg["fused_expected"] = bool(
        ranks == 1 and dim == 3 and family in FUSABLE
        and not any(s["comp"] >= 3 for s in sources) and not any(s["in_pml"] for s in sources))
    return cfg


def case_of(cfg):
    return dict(dim=cfg["dim"], n=cfg["n"], per=cfg["per"])


def _mask(cfg, box):
    """an index box over the cell's (n + 1)-point axes; modulo the period along periodic axes"""
    axes = pc.axes_of(cfg["dim"])
    shape = tuple(cfg["n"][d] + 1 for d in axes)
    m = np.ones(shape, dtype=bool)
    for k, d in enumerate(axes):
        j = np.arange(cfg["n"][d] + 1)
        s, ln = box[d]
        ok = ((j - s) % cfg["n"][d] < ln) if d in cfg["per"] else ((j >= s) & (j < s + ln))
        sh = [1] * len(shape)
        sh[k] = -1
        m &= ok.reshape(sh)
    return m


def _pos(h, nd=3):
    return [h[d] / (2 * A) for d in range(nd)]


def build(maker, cfg, R, monitors=True, fused=True):
    """cfg on maker's backend: the periodic product (R = 1, a maker with make_periodic) or a
    metal supercell of R replicas.  Returns the scene, the object and the monitors' handles."""
    sc = pc.Scene(case_of(cfg), cfg["family"], R)
    o = sc.make(maker)
    nd = len(pc.axes_of(cfg["dim"]))
    for d, side, cells in cfg["pml"]:
        o.add_pml(cells / A, dirs=(d,), sides=(side,))
    pc.materials(o, sc, _mask(cfg, cfg["block"]), _mask(cfg, cfg["slab"]))
    if hasattr(o, "make_periodic"):
        o.make_periodic(sc.per)
        if not fused:
            for f in (o._all() if hasattr(o, "_all") else [o._fields()]):
                f.set_fused(False)
    # the copies of one source in Scene.shifts() order, source after source: the order in
    # which the periodic run's lattice-shift loop makes one source's image chunks
    for src in cfg["sources"]:
        for s in sc.shifts():
            if src["kind"] == "point":
                o.add_gaussian_source(src["comp"], src["freq"], src["width"], -3.0, 3.0,
                                      tuple(p + s[d] for d, p in enumerate(_pos(src["pos"], nd))),
                                      src["amp"])
            else:
                o.add_gaussian_volume_source(
                    src["comp"], src["freq"], src["width"], -3.0, 3.0,
                    [p + s[d] for d, p in enumerate(_pos(src["lo"], nd))],
                    [p + s[d] for d, p in enumerate(_pos(src["hi"], nd))], src["amp"])
    for c in pc.D_COMPS + pc.B_COMPS:
        rng = np.random.default_rng(cfg["init_seed"] + 31 * c)
        o.initialize_field(c, sc.tile(sc.cell_array(rng, 0.1)))
    hs = {}
    if monitors:
        d = cfg["dft"]
        eh = [c for c in d["comps"] if c < 6]
        db = [c for c in d["comps"] if c >= 6]
        if eh:
            hs["eh"] = o.add_dft_fields(eh, _pos(d["lo"]), _pos(d["hi"]), FREQS, False, 1)
        if db and hasattr(o, "_fields"):  # the oracle's dft_fields take E and H only
            hs["db"] = o.add_dft_fields(db, _pos(d["lo"]), _pos(d["hi"]), FREQS, False, 1)
        f = cfg["flux"]
        hs["flux"] = o.add_dft_flux([(_pos(f["lo"]), _pos(f["hi"]), f["normal"], 1.0)], FREQS, 1)
    return sc, o, hs
