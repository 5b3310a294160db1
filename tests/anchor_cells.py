"""What the tests of kfpos_set_anchor_cells share: a layout of cells over the blocks of a bank, the inputs its tags get,
the bank with cells and its reference banks (one per group of blocks, each with ONE table under KFPOS_NO_COOP=1), the same
calls on all of them, and the byte comparison of every group's rows.

Cell c's table is the workload's anchor table with its rows rotated by c and translated by offset(c), further than the
room is wide: the tags of a block of cell c get the workload's ranges with their columns rotated alike and the workload's
start positions translated alike. Every tag then sees the geometry the workload describes -- and a block that ranged
against another cell's table would be wrong by metres and in its status words, not in last bits.

Nothing here needs a GPU on import; torch is imported where a tensor is made (step_checks.Trace)."""
import numpy as np

import step_checks
from replay_checks import env, same_bytes
from roskfpos_amd import capi
from roskfpos_amd.synth import Workload

CELL_TAGS = capi.CELL_TAGS
_OFFSETS = [(0.0, 0.0, 0.0), (64.0, -128.0, 2.0), (-37.5, 12.25, 0.5)]


def offset(c):
    """where cell c's room lies: the three of the base shape, then a spiral of rooms at least 40 m apart"""
    if c < len(_OFFSETS):
        return np.array(_OFFSETS[c])
    return np.array([40.0 * c * np.cos(c), 40.0 * c * np.sin(c), 0.25 * c])


class Layout:
    """T tags, A anchors, n_cells cells, cell_of_block[b] for every block of 64 rows"""

    def __init__(self, T, A, n_cells, cell_of_block, seed=None):
        self.T, self.A, self.n_cells = T, A, n_cells
        self.map = np.asarray(cell_of_block, dtype=np.int32)
        assert self.map.shape == ((T + CELL_TAGS - 1) // CELL_TAGS,)
        self.w = Workload(T, A) if seed is None else Workload(T, A, seed=seed)
        self.block_of_tag = np.arange(T) // CELL_TAGS
        self.offsets = np.stack([offset(c) for c in range(n_cells)])

    def perm(self, c):
        """column k of cell c is the workload's anchor perm(c)[k]"""
        return (np.arange(self.A) + c) % self.A

    def tables(self, moved=()):
        """[n_cells][A][3]; moved: cells whose anchors stand 0.75 m further along x and 0.5 m lower"""
        t = np.stack([self.w.anchors[self.perm(c)] + self.offsets[c] for c in range(self.n_cells)])
        for c in moved:
            t[c] += (0.75, 0.0, -0.5)
        return t

    def cell_of_tag(self, cell_map=None):
        return (self.map if cell_map is None else np.asarray(cell_map))[self.block_of_tag]

    def per_tag(self, a, cell_map=None):
        """a [..., T, A] in the workload's column order -> every tag's columns in its cell's order"""
        out = np.empty_like(a)
        cells = self.cell_of_tag(cell_map)
        for c in range(self.n_cells):
            out[..., cells == c, :] = a[..., cells == c, :][..., self.perm(c)]
        return out

    def init(self, cell_map=None):
        return self.w.init_positions() + self.offsets[self.cell_of_tag(cell_map)]

    def ranges(self, S, cell_map=None):
        """[S][T][A] int32, with the gaps of step_checks.Trace put in by Trace itself (gaps=True)"""
        return self.per_tag(np.stack([self.w.ranges_mm(s) for s in range(S)]), cell_map)

    def groups(self, by="block"):
        """[(name, tag mask, the block whose cell the group's reference follows)]: one group per block, or per cell"""
        if by == "block":
            return [(f"block {b}", self.block_of_tag == b, b) for b in range(self.map.size)]
        cells = self.cell_of_tag()
        return [(f"cell {c}", cells == c, int(np.flatnonzero(self.map == c)[0])) for c in sorted(set(self.map.tolist()))]


def make_bank(lay, model, storage, *, init=True, table=None, no_coop=None, **kw):
    """a bank over the layout's tags: with ONE table (table = [A][3]) or, table=None, with cell 0's until the caller
    calls set_anchor_cells. init: True = the layout's fixed starts, False = ML start"""
    ip = lay.init() if init is True else None if init is False else init
    with env(KFPOS_NO_COOP=no_coop):
        return capi.KfposBank(model, lay.T, lay.tables()[0] if table is None else table, storage=storage, init_pos=ip, **kw)


class Banks:
    """the bank with cells and one reference bank per group; call(f) runs f(bank) on every one of them and returns the
    results, the cells bank's first"""

    def __init__(self, lay, model, storage, *, by="block", init=True, cells_first=True, **kw):
        self.lay, self.groups = lay, lay.groups(by)
        self.cells = make_bank(lay, model, storage, init=init, **kw)
        if cells_first:
            self.cells.set_anchor_cells(lay.tables(), lay.map)
        tabs = lay.tables()
        self.refs = [make_bank(lay, model, storage, init=init, table=tabs[lay.map[b]], no_coop=1, **kw)
                     for _, _, b in self.groups]

    def call(self, f):
        return [f(self.cells)] + [f(r) for r in self.refs]

    def remap(self, cell_map, moved=()):
        """kfpos_set_anchor_cells again; every reference follows its block with kfpos_set_anchors"""
        tabs = self.lay.tables(moved)
        self.cells.set_anchor_cells(tabs, np.asarray(cell_map, dtype=np.int32))
        for r, (_, _, b) in zip(self.refs, self.groups):
            r.set_anchors(tabs[cell_map[b]])

    def close(self):
        for b in [self.cells] + self.refs:
            b.close()


def left(b):
    """every stored byte the accessors show: state, covariance (as stored: the accessor widens it exactly), flags, latch"""
    x, P, fl = b.get_state()
    return [x, P, fl, b.get_latch()]


LEFT = ["x", "P", "flags", "latch"]


def compare_rows(results, groups, names, what):
    """results[0]: the cells bank's arrays, results[1 + g]: group g's reference's; every array has the tags on `axis`
    given by names[i][1] -- the rows of group g must be the same bytes in both"""
    got = results[0]
    for (gname, mask, _), ref in zip(groups, results[1:]):
        assert mask.any(), gname
        same_bytes([np.ascontiguousarray(np.compress(mask, a, axis=ax)) for a, (_, ax) in zip(got, names)],
                   [np.ascontiguousarray(np.compress(mask, a, axis=ax)) for a, (_, ax) in zip(ref, names)],
                   [n for n, _ in names], f"{what}, {gname}")


SYNC_NAMES = [("status", 1), ("poses", 1)] + [(n, 0) for n in LEFT]
RUN_NAMES = [(f, {"poses": 2, "status": -1}.get(f, 0)) for f in step_checks.Run._fields]


def sync_epochs(b, tr, dts, epochs, *, rounds, per_tag_dt=None):
    """epochs through the synchronous calls -> [status [n][T], poses [n][T][3]] + left(b).
    rounds: "toa" (kfpos_step_toa), "fused" (kfpos_step_toa_imu), or "ranging9": a 9-state bank fed kfpos_step_toa only,
    with ONE kfpos_step_imu in front of epoch 2 -- epochs 0 and 1 have nothing latched, the later ones re-fuse that sample.
    per_tag_dt: {epoch: dt array [T]} (negative entries: the tag sits the epoch out)"""
    real = b.real
    err = tr.err.cpu().numpy().T.astype(real)
    cov = tr.cov_host.astype(real)
    acc = tr.accel.cpu().numpy().transpose(0, 2, 1)
    stats, poses = [], []
    for s in epochs:
        dt = (per_tag_dt or {}).get(s, dts[s])
        if rounds == "fused":
            st = b.step_toa_imu(tr.r_host[s], err, acc[s], cov, dt)
        else:
            if rounds == "ranging9" and s == 2:
                b.step_imu(acc[s], cov, 0.0)
            st = b.step_toa(tr.r_host[s], err, dt)
        stats.append(st)
        poses.append(b.get_pose(0.0)[0])
    return [np.stack(stats), np.stack(poses)] + left(b)
