"""map_bank — fixed, user-supplied maps for the envs of a handle (include/track2d_bank.h; csrc/track2d_hip.hip).

A MapBank is K square maps (uint8, 0 free / 1 wall, all-wall border, at least three free cells) with an optional start
position per map. Attached to an env before its first reset (VecTrack2D.attach_map_bank, VecEnv(map_bank=...), --map-bank),
it replaces the map generators: every episode the handle generates — inside the in-launch auto-reset too — fetches its
map tile from the bank, chosen by the header's selection rule ('cycle': (global env id + episode) mod K; 'random': one
bounded draw from the episode's MAP stream). Spawns, goals, scripted targets, rewards and the time limit are what they
were, draw for draw.

Files: .npz (maps [K, S, S] uint8, optional spawns [K, 4] int32) or .txt — one character per cell, '#' or '1' a wall, '.',
'0' or ' ' free, 'T' / 'G' free cells that start the tracker / the target there (both or neither), maps separated by
blank lines, lines starting with ';' comments.

    python -m active_tracking_rl_amd.map_bank make --env Track2D-BlockPartialPZR-v0 --count 16 --seed 7 --out held_out.npz

writes the first-episode maps of 16 generated envs: a held-out suite in one command.

There is no host path for the selection or the fetch: the library's generator kernels are the only implementation
(tests/map_bank_spec.py restates the rule in plain Python for the tests)."""
import argparse
import ctypes as C
import sys

import numpy as np

CYCLE, RANDOM = 0, 1            # T2D_BANK_CYCLE, T2D_BANK_RANDOM
SELECT = {"cycle": CYCLE, "random": RANDOM}
MAX_MAPS = 65536                # T2D_BANK_MAX_MAPS
MIN_FREE = 3                    # sample_goal(2) and the goal-test loop need three free cells
SIDES = (81, 82)                # Maze; Block / Empty
NO_SPAWN = (-1, -1, -1, -1)

_P = C.c_void_p
# {entry point: (restype, [argtypes])} for every function include/track2d_bank.h declares
BANK_PROTOTYPES = {
    "t2d_map_bank_attach": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "t2d_map_bank_index": (C.c_int, [_P, _P, _P]),
    "t2d_map_bank_count": (C.c_int, [_P]),
}
_STATUS = ("t2d_map_bank_attach", "t2d_map_bank_index")      # (t2d_map_bank_count returns K)
_lib = None


def _errcheck(name):
    """As occlusion._errcheck, with vec_env's exception: a non-zero status raises T2DError naming the entry point, with the
    library's own text."""
    def check(status, func=None, args=None):
        if status != 0:
            from . import vec_env
            raise vec_env.T2DError("%s failed (%d): %s" % (name, status, vec_env.load_library().t2d_last_error().decode()))
        return status
    return check


def lib():
    global _lib
    if _lib is None:
        from . import vec_env
        L = vec_env.load_library()
        for name, (restype, argtypes) in BANK_PROTOTYPES.items():
            f = getattr(L, name)         # (a library without the symbol is an error: there is no other path)
            f.restype, f.argtypes = restype, argtypes
            if name in _STATUS:
                f.errcheck = _errcheck(name)
        _lib = L
    return _lib


def map_fault(m, i=0):
    """Why map `m` ([S, S] integers) cannot be a bank member, in the library's words, or None."""
    side = m.shape[0]
    bad = np.argwhere(m > 1)
    if len(bad):
        r, c = (int(v) for v in bad[0])
        return "map %d: cell (%d, %d) is %d, not 0 / 1" % (i, r, c, int(m[r, c]))
    border = np.ones_like(m, bool)
    border[1:-1, 1:-1] = False
    bad = np.argwhere(border & (m == 0))
    if len(bad):
        return "map %d: border cell (%d, %d) is not a wall" % (i, int(bad[0][0]), int(bad[0][1]))
    n_free = int((m == 0).sum())
    if n_free < MIN_FREE:
        return "map %d: %d free cell(s), at least %d are needed" % (i, n_free, MIN_FREE)
    return None


def spawn_fault(m, row, i=0):
    """Why spawn row `row` (four integers) cannot go with map `m`, or None: all -1, or two free in-map cells."""
    p = tuple(int(v) for v in row)
    if p == NO_SPAWN:
        return None
    if any(v < 0 or v >= m.shape[0] for v in p):
        return "map %d: spawn row (%d, %d, %d, %d) is neither all -1 nor inside the map" % ((i,) + p)
    if m[p[0], p[1]] or m[p[2], p[3]]:
        return "map %d: spawn row (%d, %d, %d, %d) places an agent on a wall" % ((i,) + p)
    return None


class MapBank(object):
    """K maps [K, S, S] uint8 (0 free / 1 wall) and, optionally, spawns [K, 4] int32 = {tracker r, c, target r, c} per map
    (a row of four -1: sample as usual). ValueError names the first map that cannot be a member, and why."""

    def __init__(self, maps, spawns=None):
        maps = np.asarray(maps)
        if maps.ndim == 2:
            maps = maps[None]
        if maps.ndim != 3 or maps.shape[1] != maps.shape[2] or maps.shape[1] < 3:
            raise ValueError("MapBank: maps must be [K, S, S] with S >= 3, got shape %s" % (tuple(maps.shape),))
        if maps.dtype.kind not in "biu":
            raise ValueError("MapBank: maps must be integers (0 free / 1 wall), got %s" % (maps.dtype,))
        if not 1 <= maps.shape[0] <= MAX_MAPS:
            raise ValueError("MapBank: count %d outside 1 .. %d" % (maps.shape[0], MAX_MAPS))
        if maps.shape[1] > max(SIDES):
            raise ValueError("MapBank: side %d, the envs' maps have side %d (Maze) or %d" % (maps.shape[1], SIDES[0], SIDES[1]))
        if maps.dtype.kind == "i" and (maps < 0).any():
            i, r, c = (int(v) for v in np.argwhere(maps < 0)[0])
            raise ValueError("MapBank: map %d: cell (%d, %d) is %d, not 0 / 1" % (i, r, c, int(maps[i, r, c])))
        for i in range(maps.shape[0]):
            why = map_fault(maps[i], i)
            if why:
                raise ValueError("MapBank: " + why)
        self.maps = np.ascontiguousarray(maps, np.uint8)
        self.spawns = None
        if spawns is not None:
            spawns = np.asarray(spawns)
            if spawns.shape != (self.count, 4) or spawns.dtype.kind not in "iu":
                raise ValueError("MapBank: spawns must be integers [%d, 4], got %s %s" % (self.count, spawns.dtype, tuple(spawns.shape)))
            for i in range(self.count):
                why = spawn_fault(self.maps[i], spawns[i], i)
                if why:
                    raise ValueError("MapBank: " + why)
            self.spawns = np.ascontiguousarray(spawns, np.int32)

    @property
    def count(self):
        return int(self.maps.shape[0])

    @property
    def side(self):
        return int(self.maps.shape[1])

    def __len__(self):
        return self.count

    def fit(self, side):
        """The bank at the handle's side: walls added at the bottom and right (cells and spawn rows keep their coordinates).
        A map larger than `side` is refused."""
        side = int(side)
        if self.side > side:
            raise ValueError("MapBank.fit: the maps have side %d, larger than %d" % (self.side, side))
        if self.side == side:
            return self
        maps = np.ones((self.count, side, side), np.uint8)
        maps[:, :self.side, :self.side] = self.maps
        return MapBank(maps, self.spawns)

    # -- files ----------------------------------------------------------------------------------------------
    def save(self, path):
        path = str(path)
        if path.endswith(".npz"):
            arrays = dict(maps=self.maps)
            if self.spawns is not None:
                arrays["spawns"] = self.spawns
            with open(path, "wb") as f:          # (a file object: np.savez appends no second suffix)
                np.savez_compressed(f, **arrays)
        elif path.endswith(".txt"):
            with open(path, "w") as f:
                f.write(self.to_text())
        else:
            raise ValueError("MapBank.save: %r is neither .npz nor .txt" % (path,))
        return path

    @classmethod
    def load(cls, path):
        path = str(path)
        if path.endswith(".npz"):
            with np.load(path) as z:
                if "maps" not in z.files:
                    raise ValueError("MapBank.load: %r has no 'maps' array" % (path,))
                return cls(z["maps"], z["spawns"] if "spawns" in z.files else None)
        if path.endswith(".txt"):
            with open(path) as f:
                return cls.from_text(f.read())
        raise ValueError("MapBank.load: %r is neither .npz nor .txt" % (path,))

    def to_text(self):
        out = ["; %d map(s) of side %d: '#' wall, '.' free, 'T' tracker start, 'G' target start" % (self.count, self.side)]
        for i in range(self.count):
            rows = [["#" if v else "." for v in row] for row in self.maps[i]]
            if self.spawns is not None and tuple(self.spawns[i]) != NO_SPAWN:
                tr, tc, gr, gc = (int(v) for v in self.spawns[i])
                if (tr, tc) == (gr, gc):
                    raise ValueError("MapBank.to_text: map %d starts both agents on (%d, %d), which the .txt marks cannot say "
                                     "(save as .npz)" % (i, tr, tc))
                rows[tr][tc], rows[gr][gc] = "T", "G"
            out.append("\n".join("".join(r) for r in rows))
        return "\n\n".join(out) + "\n"

    @classmethod
    def from_text(cls, text):
        blocks, cur = [], []
        for line in text.splitlines():
            if line.startswith(";"):
                continue
            if line.strip() == "":
                if cur:
                    blocks.append(cur)
                cur = []
            else:
                cur.append(line.rstrip("\r\n"))
        if cur:
            blocks.append(cur)
        if not blocks:
            raise ValueError("MapBank.from_text: no map found")
        maps, spawns = [], []
        for i, rows in enumerate(blocks):
            width = len(rows[0])
            if any(len(r) != width for r in rows):
                raise ValueError("MapBank.from_text: map %d has ragged rows" % i)
            if len(rows) != width:
                raise ValueError("MapBank.from_text: map %d is %d x %d, not square" % (i, len(rows), width))
            m = np.zeros((width, width), np.uint8)
            marks = {}
            for r, row in enumerate(rows):
                for c, ch in enumerate(row):
                    if ch in "#1":
                        m[r, c] = 1
                    elif ch in "TG":
                        if ch in marks:
                            raise ValueError("MapBank.from_text: map %d has more than one %r" % (i, ch))
                        marks[ch] = (r, c)
                    elif ch not in ".0 ":
                        raise ValueError("MapBank.from_text: map %d: character %r at (%d, %d)" % (i, ch, r, c))
            if len(marks) == 1:
                raise ValueError("MapBank.from_text: map %d has %r but no %r: a spawn row needs both"
                                 % (i, list(marks)[0], "G" if "T" in marks else "T"))
            maps.append(m)
            spawns.append(marks["T"] + marks["G"] if marks else NO_SPAWN)
        if len(set(m.shape for m in maps)) != 1:
            raise ValueError("MapBank.from_text: the maps have different sides %s" % (sorted(set(m.shape[0] for m in maps)),))
        has_spawns = any(s != NO_SPAWN for s in spawns)
        return cls(np.stack(maps), np.array(spawns, np.int32) if has_spawns else None)

    # -- generated banks -------------------------------------------------------------------------------------
    @classmethod
    def from_env(cls, env_id, count, seed=1, device="cuda:0"):
        """The first-episode maps of `count` generated envs of `env_id` (reset + get_maps), at the id's own side."""
        from .vec_env import VecTrack2D
        env = VecTrack2D(env_id, num_envs=int(count), device=device, seed=seed)
        try:
            env.reset()
            side = int(env.get_state(0, 1)["side"][0])
            return cls(env.get_maps()[:, :side, :side])
        finally:
            env.close()


def as_bank(bank):
    """A MapBank from a MapBank, a file name or a [K, S, S] array."""
    if isinstance(bank, MapBank):
        return bank
    if isinstance(bank, str):
        return MapBank.load(bank)
    return MapBank(bank)


def select_code(select):
    if select not in SELECT:
        raise ValueError("map bank: select %r, expected 'cycle' or 'random'" % (select,))
    return SELECT[select]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m active_tracking_rl_amd.map_bank", description="Map bank files (.npz / .txt).")
    sub = ap.add_subparsers(dest="cmd")
    mk = sub.add_parser("make", help="write the first-episode maps of COUNT generated envs as a bank")
    mk.add_argument("--env", required=True, metavar="ID", help="a Track2D id, e.g. Track2D-BlockPartialPZR-v0")
    mk.add_argument("--count", type=int, required=True, metavar="K")
    mk.add_argument("--seed", type=int, default=1, metavar="S")
    mk.add_argument("--out", required=True, metavar="FILE", help=".npz or .txt")
    mk.add_argument("--device", default="cuda:0")
    sh = sub.add_parser("show", help="print a bank file's size and its maps' free-cell counts")
    sh.add_argument("file")
    args = ap.parse_args(argv)
    if args.cmd == "make":
        bank = MapBank.from_env(args.env, args.count, seed=args.seed, device=args.device)
        print("%s: %d map(s) of side %d" % (bank.save(args.out), bank.count, bank.side))
    elif args.cmd == "show":
        bank = MapBank.load(args.file)
        print("%s: %d map(s) of side %d, %s" % (args.file, bank.count, bank.side,
                                                "no spawn rows" if bank.spawns is None else
                                                "%d spawn row(s)" % int((bank.spawns != -1).all(1).sum())))
        for i in range(bank.count):
            print("  map %d: %d free cells" % (i, int((bank.maps[i] == 0).sum())))
    else:
        ap.print_help()
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
