"""Env-id table: restates the registry loop of the reference (envs/gym-track2d/gym_track2d/__init__.py:3-18):
72 ids `Track2D-{Maze,Block,Empty}{Full,Partial}{Adv,PZR,Far,Nav,Ram,RPF}-v{0,1}`, each with
max_episode_steps=500. All 72 are built (`RPF` = the Navigator patrolling the four static goal cells,
generators.py:12-19).

Beside the table, `spec()` resolves by rule the ids of this project's own generated map type,
`Track2D-Rooms{Full,Partial}{Adv,PZR,Far,Nav,Ram}-v{0..15}` (include/track2d.h T2D_MAP_ROOMS: rooms joined by doorways; the
level sets the smallest room side, 3 + 2 level, level 0 draws it per episode). There is no Rooms id with the RPF target."""
import re

MAP_TYPES = ("Maze", "Block", "Empty")
OBS_TYPES = ("Full", "Partial")
TARGET_MODES = ("Adv", "PZR", "Far", "Nav", "Ram", "RPF")
MAX_EPISODE_STEPS = 500

MAP_CODE = {"Block": 0, "Maze": 1, "Empty": 2, "Rooms": 3}
TARGET_CODE = {"Adv": 0, "PZR": 1, "Far": 2, "Nav": 3, "Ram": 4, "RPF": 5,
               "Ext": 6}   # not an id: target action supplied by the caller (include/track2d.h T2D_TGT_EXT)

REGISTRY = {}
for _m in MAP_TYPES:
    for _o in OBS_TYPES:
        for _t in TARGET_MODES:
            for _l in range(2):
                REGISTRY["Track2D-%s%s%s-v%d" % (_m, _o, _t, _l)] = dict(
                    map_type=_m, obs_type=_o, level=_l, target_mode=_t, max_episode_steps=MAX_EPISODE_STEPS)

ROOMS_TARGET_MODES = ("Adv", "PZR", "Far", "Nav", "Ram")
ROOMS_MAX_LEVEL = 15
_ROOMS_ID = re.compile(r"^Track2D-Rooms(%s)(%s)-v(0|[1-9][0-9]?)$" % ("|".join(OBS_TYPES), "|".join(ROOMS_TARGET_MODES)))


def is_rooms(env_id):
    """True for an id that resolves to the Rooms map type."""
    m = _ROOMS_ID.match(env_id) if isinstance(env_id, str) else None
    return m is not None and int(m.group(3)) <= ROOMS_MAX_LEVEL


def spec(env_id):
    if env_id in REGISTRY:
        return dict(REGISTRY[env_id])
    if is_rooms(env_id):
        o, t, l = _ROOMS_ID.match(env_id).groups()
        return dict(map_type="Rooms", obs_type=o, level=int(l), target_mode=t, max_episode_steps=MAX_EPISODE_STEPS)
    raise KeyError("unknown env id %r (72 Track2D ids are registered; Track2D-Rooms{Full,Partial}{Adv,PZR,Far,Nav,Ram}-v{0..15} "
                   "resolve by rule)" % (env_id,))
