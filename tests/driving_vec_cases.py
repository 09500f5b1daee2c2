"""The Driving-v1 step cases shared by tests/test_driving_vec_host.py (CPU: the
host build of csrc/driving_vec.h against the scalar functions of driving.h) and
tests/test_gpu_env_step_selftest.py (GPU: pomcp_debug_env_step against the host
model), on the 14x14RoundAbout grid.

A case is (s0, s1, a0, a1, j): two packed vehicles (driving.h), their actions
and the execution-order draw (0: vehicle 1 moves first).  Three tiers:

  1. vehicle 0 in every (free cell, heading, speed) with every action and both
     draws, vehicle 1 far away;
  2. the same sweep with vehicle 1 on the first cell ahead of vehicle 0's
     heading, on the second, and adjacent but off that line (a turn or a reverse
     speed puts these on the path of the move instead), both draws; vehicle 1
     faces vehicle 0 at full speed or backs towards it, and its own action runs
     through every value;
  3. every (free cell, heading) of vehicle 0 with every destination, the flags
     none / reached / crashed on either vehicle, and the min-distance field 0 /
     its cell's distance / 127, vehicle 1 on the first cell ahead or far away.

The reward table covers a progress of 0..2 cells (driving.h prog): a vehicle
that is not done and holds more than its cell's distance would index past it,
in the host model (drv_reward_fast) just as on the device.  So 127 goes to the
vehicle that carries a flag; with no flag set the case keeps the cell's
distance, the largest value inside the table.
"""
import numpy as np

DX = (0, 1, 0, -1)
DY = (-1, 0, 1, 0)


def pack(x, y, d, sp, dest, reached, crashed, mind, initd):
    return (x | (y << 4) | (d << 8) | (sp << 10) | (dest << 12) | (reached << 15) | (crashed << 16)
            | (mind << 17) | (initd << 24))


def driving_cases(model):
    """uint32 [N, 5] rows (s0, s1, a0, a1, j) for a DrivingModel."""
    w, h, wall, dist = model.width, model.height, model._wall, model._dist
    nloc = len(model.locs)

    def free(x, y):
        return 0 <= x < w and 0 <= y < h and not wall[y][x]

    cells = [(x, y) for y in range(h) for x in range(w) if free(x, y)]

    def veh(x, y, d, sp, dest, flag=0, mind=None):
        cur = dist[dest][y][x]
        return pack(x, y, d, sp, dest, int(flag == 1), int(flag == 2), cur if mind is None else mind,
                    min(127, max(1, cur + 3)))

    def far(x, y):
        return max(cells, key=lambda c: (abs(c[0] - x) + abs(c[1] - y), c))

    def place(x, y, d, kind):
        """Vehicle 1's cell and the direction it lies in from vehicle 0."""
        k = (d + 1) & 3 if kind == 2 else d
        n = 2 if kind == 1 else 1
        ok = kind < 3 and all(free(x + i * DX[k], y + i * DY[k]) for i in range(1, n + 1))
        return ((x + n * DX[k], y + n * DY[k]), k) if ok else (far(x, y), d)

    rows = []
    n = 0
    for (x, y) in cells:                      # tier 1
        for d in range(4):
            for sp in range(4):
                for a0 in range(5):
                    for j in range(2):
                        (ox, oy), _ = place(x, y, d, 3)
                        rows.append((veh(x, y, d, sp, 0), veh(ox, oy, (d + 1) & 3, 2, 3), a0, n % 5, j))
                        n += 1
    for (x, y) in cells:                      # tier 2
        for d in range(4):
            for sp in range(4):
                for a0 in range(5):
                    for kind in range(3):
                        for j in range(2):
                            (ox, oy), k = place(x, y, d, kind)
                            back = (n // 5) % 2
                            s1 = veh(ox, oy, k if back else (k + 2) & 3, 0 if back else 3, 3)
                            rows.append((veh(x, y, d, sp, 0), s1, a0, n % 5, j))
                            n += 1
    flags = ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2))
    for (x, y) in cells:                      # tier 3
        for d in range(4):
            for dest in range(nloc):
                for (f0, f1) in flags:
                    for mv in range(3):
                        (ox, oy), k = place(x, y, d, 0 if n % 2 == 0 else 3)
                        m0 = m1 = None
                        if mv == 0:
                            m0 = 0
                        elif mv == 2 and f0 != 0:
                            m0 = 127
                        elif mv == 2 and f1 != 0:
                            m1 = 127
                        s0 = veh(x, y, d, 2 + (n // 4) % 2, dest, f0, m0)
                        s1 = veh(ox, oy, (k + 2) & 3, 3, (dest + 3) % nloc, f1, m1)
                        rows.append((s0, s1, (n // 8) % 5, (n // 40) % 5, (n // 2) % 2))
                        n += 1
    return np.array(rows, dtype=np.uint32)
