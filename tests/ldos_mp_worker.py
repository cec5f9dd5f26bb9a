"""One rank of the multi-process LDOS run (tests/test_gpu_ldos_mp.py), after tests/mp_worker.py:

  python tests/ldos_mp_worker.py RANK NRANKS ID_HEX OUT_DIR

The x-z plane source of test_gpu_ldos on z-slabs, one process per slab; writes
OUT_DIR/ldos.rank<R>.npz with what ldos_data returns on this rank (a collective: the same on
every rank), the point list and the transport."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from mp_worker import make_dist  # noqa: E402
import test_gpu_ldos as T  # noqa: E402


def main():
    rank, nranks = int(sys.argv[1]), int(sys.argv[2])
    nid, out = bytes.fromhex(sys.argv[3]), sys.argv[4]
    o = T._cell(make_dist(rank, nranks, nid), 3, T.BOX3, T._src_xz_plane)
    f = o._fields()
    h = f.add_ldos(T.FREQS)
    comp, ijk, amp = f.ldos_points(h)
    T._run_recorded(o, h, (1, T.STEPS - 1))
    ld, F, J, scale = f.ldos_data(h)
    np.savez(os.path.join(out, f"ldos.rank{rank}.npz"), ldos=ld, F=F, J=J, scale=np.array([scale]),
             comp=comp, ijk=ijk, amp=amp, transport=np.array(f.transport()),
             fused=np.array([f.fused_active()]), t=np.array([o.t]))
    print(f"rank {rank}: ldos done", flush=True)


if __name__ == "__main__":
    main()
