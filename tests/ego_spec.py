"""The rule of include/atr_ego.h in plain numpy loops, one cell at a time, written from the header's text (not from the kernels and
not from csrc/atr_ego_rule.h): the reference of the egocentric-view tests. The turn rule is the field of view's (fov_spec.turn)."""
import numpy as np

from fov_spec import NONE, turn, turn_all  # noqa: F401  (the heading turns by the field of view's rule, unchanged)

SIDE, WINDOW, CENTRE = 13, 169, 6
MOVES = {0: (-1, 0), 1: (1, 0), 2: (0, -1), 3: (0, 1)}      # (ur, uc) of a heading; the same four as absolute moves
FORWARD, BACK, LEFT, RIGHT = 0, 1, 2, 3
ABS = ((0, 1, 2, 3), (1, 0, 3, 2), (2, 3, 1, 0), (3, 2, 0, 1))       # ABS[heading][relative action], as the header prints it
REL = tuple(tuple(row.index(a) for a in range(4)) for row in ABS)    # the inverse of every row
FACINGS = (0, 1, 2, 3, NONE, 7)         # 7: a value that is no facing
ROLES = {"tracker": 1, "target": 2, "both": 3}


def heading_of(facing):
    """NONE, and any value that is no facing, counts as heading 0."""
    return int(facing) if 0 <= int(facing) <= 3 else 0


def to_abs(facing, k):
    """The absolute action of relative action k; an action outside 0 .. 3 passes through."""
    return ABS[heading_of(facing)][int(k)] if 0 <= int(k) <= 3 else int(k)


def to_rel(facing, a):
    return REL[heading_of(facing)][int(a)] if 0 <= int(a) <= 3 else int(a)


def source(heading, r, c):
    """(row, column) of the absolute window that cell (r, c) of the egocentric window shows."""
    ur, uc = MOVES[heading]
    er, ec = r - CENTRE, c - CENTRE
    dr, dc = -er * ur + ec * uc, -er * uc - ec * ur
    return CENTRE + dr, CENTRE + dc


def view(window, facing):
    """The egocentric window [13, 13] of an absolute window under a facing byte."""
    w = np.asarray(window)
    assert w.shape == (SIDE, SIDE)
    h = heading_of(facing)
    out = np.empty_like(w)
    for r in range(SIDE):
        for c in range(SIDE):
            out[r, c] = w[source(h, r, c)]
    return out


def view_all(windows, facing, roles=3):
    """A copy of windows [N, P, 13, 13] with the window of every player in `roles` turned by facing[e, p]."""
    w = np.asarray(windows)
    f = np.asarray(facing)
    assert w.ndim == 4 and f.shape == w.shape[:2]
    out = w.copy()
    for e in range(w.shape[0]):
        for p in range(w.shape[1]):
            if (roles >> p) & 1:
                out[e, p] = view(w[e, p], f[e, p])
    return out


def abs_all(facing, rel, roles=3):
    """facing [N, 2], rel = (r0 [N], r1 [N] or None) -> the absolute actions, per player an int64 array (None where rel's is)."""
    out = []
    for p, r in enumerate(rel):
        if r is None:
            out.append(None)
            continue
        r = np.asarray(r).astype(np.int64)
        out.append(np.array([to_abs(facing[e, p], r[e]) if (roles >> p) & 1 else int(r[e]) for e in range(len(r))], np.int64))
    return out


def turn_roles(facing, actions=(None, None), done=None, roles=3):
    """fov_spec.turn_all for the players in `roles`; the bytes of the others stay."""
    f = np.array(facing, np.uint8)
    new = turn_all(f, actions, done)
    for p in range(f.shape[1]):
        if (roles >> p) & 1:
            f[:, p] = new[:, p]
    return f


def windows_call(windows, facing, actions=(None, None), done=None, roles=3):
    """One call of atr_ego_windows: (turned windows, new facing)."""
    f = turn_roles(facing, actions, done, roles)
    return view_all(windows, f, roles), f


class EnvModel(object):
    """A step-by-step model of an egocentric env's facing bytes [N, 2], from what a plain twin reports. roles: the egocentric
    players; scripted: the target takes no action of a player (its byte never turns); fov: a field-of-view pass turns the bytes
    of every player whose actions reach it (both, or the tracker alone where the target is scripted) — else only the egocentric
    players' bytes turn; auto_reset: the core's done flags reach the passes."""

    def __init__(self, n, roles=3, scripted=False, fov=False, auto_reset=True):
        self.n, self.roles, self.scripted, self.fov, self.auto_reset = n, roles, scripted, fov, auto_reset
        self.reset()

    def reset(self):
        self.facing = np.full((self.n, 2), NONE, np.uint8)

    def absolute(self, rel):
        """rel = (r0 [N], r1 [N] or None): the absolute actions of the step that starts from the standing heading."""
        return abs_all(self.facing, rel, self.roles)

    def stepped(self, abs_actions, done):
        """The step ran with abs_actions and reported done: the bytes turn, once."""
        a0, a1 = abs_actions
        acts = (a0, None if self.scripted else a1)
        roles = (1 if self.scripted else 3) if self.fov else self.roles
        self.facing = turn_roles(self.facing, acts, done if self.auto_reset else None, roles)

    def see(self, windows):
        """The twin's windows [N, 2, 13, 13] (after its own passes) -> what the egocentric env hands out."""
        return view_all(windows, self.facing, self.roles)
