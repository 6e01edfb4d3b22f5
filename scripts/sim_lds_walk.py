#!/usr/bin/env python3
"""CPU model of the closest-hit link walk of an LDS-resident scene (closest_small_links, rtx_kernels.h) in its forms - host library only, no device:
SPEC 0: a lane that holds a leaf sits out the node rounds; 1: it walks on with the t_max it has and stalls at the next leaf whose box it passes (built: k_trace_spec<1>);
2: it may remember one such leaf and stalls at the second - the remembered leaf takes the held one's place after a second box test if t_max shrank since; 3: as 2, the
second box test taken in the next node round instead (2 and 3: built, exact, measured and not kept - MEASUREMENTS R9). The model walks the kernel's state machine over HostScene.link_tables() (the kept rows), 64 rays to a wave, with a float64 slab
test and a float64 Moller-Trumbore triangle test in place of the device's, and counts node rounds, leaf phases and tests.

Usage: scripts/sim_lds_walk.py [scene] [LEAF_MIN ...]      scene: cornell (default) | soup-126 | soup-40-degenerate
Rays: 1536 five-deep random-walk chains from uniform points inside the scene's bounds; a wave is 64 rays of one bounce. Cost: 34 instructions per node round, 70 per
leaf phase (DESIGN 5.3's figures for the as-built kernel; the bookkeeping the forms add per round is NOT in the model)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_ROUND_COST, LEAF_PHASE_COST = 34, 70
INF = float("inf")


def scene_desc(name):
    from rustracer_amd.scenes import cornell_box, random_soup
    if name == "cornell":
        return cornell_box(8, 8, 1)
    if name == "soup-126":
        return random_soup(126, seed=5, max_prims=4)
    if name == "soup-40-degenerate":
        return random_soup(40, seed=9, max_prims=1, degenerate=True)
    raise ValueError(name)


class Model:
    """The tables the kernel stages: node bounds, the kept link rows with their start nodes, the triangles in leaf order."""

    def __init__(self, desc):
        from rustracer_amd import host
        h = host.HostScene(desc)
        b, lt = h.bvh(), h.link_tables()
        P, idx = desc.arrays()[:2]
        self.lo, self.hi = b["bounds"][:, :3].astype(np.float64), b["bounds"][:, 3:].astype(np.float64)
        self.n_nodes = len(b["offset"])
        self.tris = P[idx[b["ordered"]]].astype(np.float64)      # [leaf slot][vertex][xyz]
        self.n_prims = len(self.tris)
        self.rows = [[int(w) for w in lt["kept"][o]] for o in range(8)]
        self.starts = [int(s) for s in lt["start_kept"][:8]]

    def leaf_fields(self, word):
        return (word >> 16) & 0x7f, (word & 0x7fffffff) >> 23   # RT_LINK_LEAF_OFF / RT_LINK_LEAF_N of the 256-node kernels

    def prepare(self, org, d):
        """Per ray what the tests need that does not depend on t_max: per node (box passed for t_max = inf, entry distance), per primitive the hit distance or inf."""
        out = []
        e1, e2, v0 = self.tris[:, 1] - self.tris[:, 0], self.tris[:, 2] - self.tris[:, 0], self.tris[:, 0]
        for o, w in zip(np.asarray(org, np.float64), np.asarray(d, np.float64)):
            inv = 1.0 / w
            a0, a1 = (self.lo - o) * inv, (self.hi - o) * inv
            tn, tf = np.minimum(a0, a1).max(1), np.maximum(a0, a1).min(1)
            geo = (tn <= tf) & (tf > 0)
            p = np.cross(w, e2)
            det = (e1 * p).sum(1)
            ok = np.abs(det) > 1e-300
            idet = 1.0 / np.where(ok, det, 1.0)
            s = o - v0
            u = (s * p).sum(1) * idet
            qv = np.cross(s, e1)
            v = (qv * w).sum(1) * idet
            t = (e2 * qv).sum(1) * idet
            ok &= (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
            octant = int(w[0] < 0) | (int(w[1] < 0) << 1) | (int(w[2] < 0) << 2)
            out.append((geo.tolist(), tn.tolist(), np.where(ok, t, INF).tolist(), octant))
        return out


def walk_wave(m, rays, t_caps, spec, leaf_min):
    """One wave (<= 64 prepared rays) through closest_small_links<.., SPEC>. Returns (per ray: final leaf slot or -1, final t_max, [(leaf slot, t_max at its test), ...]),
    dict(node_rounds, node_lanes, leaf_phases, node_tests, tri_tests)."""
    n, nn = len(rays), m.n_nodes
    assert 1 <= n <= 64
    link = [m.rows[r[3]] for r in rays]
    cur = [m.starts[r[3]] for r in rays]
    leaf_off, leaf_n, stalled = [0] * n, [0] * n, [False] * n
    q, changed, back = [-1] * n, [False] * n, [-1] * n
    t_max, prim, log = list(t_caps), [-1] * n, [[] for _ in range(n)]
    st = dict(node_rounds=0, node_lanes=0, leaf_phases=0, node_tests=0, tri_tests=0)

    def can_step(i):
        return cur[i] < nn and (leaf_n[i] == 0 if spec == 0 else not stalled[i])

    def box(i, node):
        st["node_tests"] += 1
        return rays[i][0][node] and rays[i][1][node] < t_max[i]

    while True:
        while True:
            steppers = [i for i in range(n) if can_step(i)]
            for i in steppers:
                c = cur[i]
                w = link[i][c]
                nxt = w & 0xffff
                if box(i, c):
                    if w >> 31:
                        if leaf_n[i] == 0:
                            leaf_off[i], leaf_n[i] = m.leaf_fields(w)
                        elif spec in (2, 3) and q[i] < 0:
                            q[i], changed[i] = c, False
                        else:
                            nxt, stalled[i] = c, True
                    else:
                        nxt = w >> 16
                if back[i] >= 0:            # SPEC 3: that was the remembered leaf's second test - back to where the walk stood
                    nxt, back[i] = back[i], -1
                cur[i] = nxt
            if steppers:
                st["node_rounds"] += 1
                st["node_lanes"] += len(steppers)
            holders = sum(1 for i in range(n) if leaf_n[i] > 0)
            if not any(can_step(i) for i in range(n)) or holders >= leaf_min:
                break
        if holders == 0:
            break
        st["leaf_phases"] += 1
        for i in range(n):
            if leaf_n[i] == 0:
                continue
            t = leaf_off[i]
            st["tri_tests"] += 1
            log[i].append((t, t_max[i]))
            th = rays[i][2][t]
            if th < t_max[i]:
                t_max[i], prim[i], changed[i] = th, t, True
            leaf_off[i] += 1
            leaf_n[i] -= 1
            if leaf_n[i] == 0:
                if spec == 2 and q[i] >= 0:
                    if not changed[i] or box(i, q[i]):
                        leaf_off[i], leaf_n[i] = m.leaf_fields(link[i][q[i]])
                    q[i] = -1
                stalled[i] = False
                if spec == 3 and q[i] >= 0:   # the remembered leaf is next in link order: the coming node round tests its box under the t_max of now
                    cur[i], back[i], q[i] = q[i], cur[i], -1
    return [(prim[i], t_max[i], log[i]) for i in range(n)], st


def brute_force(prep, t_cap):
    """(leaf slot of the closest primitive or -1, its distance)"""
    t = np.asarray(prep[2])
    k = int(np.argmin(t))
    return (k, float(t[k])) if t[k] < t_cap else (-1, t_cap)


def random_walk_rays(m, n_chains, depth, seed=1):
    """[bounce][chain] (origin, direction): chains of `depth` rays, each from the previous hit into a uniform direction of the hemisphere on the ray's side."""
    rng = np.random.default_rng(seed)
    org = rng.uniform(m.lo[0], m.hi[0], (n_chains, 3))
    d = rng.normal(size=(n_chains, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    alive = np.ones(n_chains, bool)
    bounces = []
    for _ in range(depth):
        k = np.nonzero(alive)[0]
        if not len(k):
            break
        prep = m.prepare(org[k], d[k])
        bounces.append((org[k].copy(), d[k].copy(), prep))
        for j, i in enumerate(k):
            p, t = brute_force(prep[j], INF)
            if p < 0:
                alive[i] = False
                continue
            tri = m.tris[p]
            ng = np.cross(tri[1] - tri[0], tri[2] - tri[0])
            ng /= max(np.linalg.norm(ng), 1e-300)
            if ng @ d[i] > 0:
                ng = -ng
            w = rng.normal(size=3)
            w /= np.linalg.norm(w)
            if w @ ng < 0:
                w = -w
            org[i] = org[i] + t * d[i] + 1e-6 * np.linalg.norm(m.hi[0] - m.lo[0]) * ng
            d[i] = w
    return bounces


def table(scene="cornell", thresholds=(16, 24), chains=1536, depth=5):
    m = Model(scene_desc(scene))
    bounces = random_walk_rays(m, chains, depth)
    n_rays = sum(len(b[2]) for b in bounces)
    print(f"{scene}: {m.n_nodes} nodes, {m.n_prims} primitives, {n_rays} rays in waves of 64")
    print(f"{'SPEC':>4} {'LEAF_MIN':>8} {'node rounds/wave':>17} {'lanes/node round':>17} {'leaf phases':>12} {'node tests/ray':>15} {'tri tests/ray':>14} {'cost/wave':>10}")
    final = {}
    for spec in (0, 1, 2, 3):
        for lm in thresholds:
            tot, waves, prims = dict(node_rounds=0, node_lanes=0, leaf_phases=0, node_tests=0, tri_tests=0), 0, []
            for _, _, prep in bounces:
                for a in range(0, len(prep), 64):
                    res, st = walk_wave(m, prep[a:a + 64], [INF] * len(prep[a:a + 64]), spec, lm)
                    prims += [r[0] for r in res]
                    waves += 1
                    for k in tot:
                        tot[k] += st[k]
            final[(spec, lm)] = prims
            cost = (NODE_ROUND_COST * tot["node_rounds"] + LEAF_PHASE_COST * tot["leaf_phases"]) / waves
            print(f"{spec:4d} {lm:8d} {tot['node_rounds'] / waves:17.1f} {tot['node_lanes'] / max(tot['node_rounds'], 1):17.1f} {tot['leaf_phases'] / waves:12.1f} "
                  f"{tot['node_tests'] / n_rays:15.2f} {tot['tri_tests'] / n_rays:14.2f} {cost:10.0f}")
    same = all(v == final[(0, thresholds[0])] for v in final.values())
    print("every ray found the same primitive in all forms" if same else "THE FORMS DISAGREE ON SOME RAY'S PRIMITIVE")
    return same


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    args = sys.argv[1:]
    sys.exit(0 if table(args[0] if args else "cornell", tuple(int(a) for a in args[1:]) or (16, 24)) else 1)
