"""Names for the step's optional contact report (`hrl_buffers_ext.contacts`, `BatchedEnv.record_contacts()`): what the reference reads with
`p.getContactPoints(...)` after `stepSimulation()` (ant_gather_env.py:113-116, gather_base.py:103-106).

The raw tensor is [N, 256] float32, one fixed record per env (layout: include/hrl_envs.h).  `decode` slices it into named views and a
few cheap torch ops on whatever device the tensor lives on -- no host round trip --, `link_force` sums the contact forces per body."""
import torch

from . import _capi as K

GROUND, WALL, BOX, ITEM, SELF = 0, 1, 2, 3, 4   # decode()['kind']; -1 in the slots beyond an env's contacts


def decode(raw, cfg=None):
    """raw: [N, HRL_CONTACTS_STRIDE] float32 as the step wrote it (`cfg`, when given, is only checked against its shape).  Returns a dict:
        n [N] int32, valid [N, 12] bool (slot < n),
        position, normal [N, 12, 3], distance [N, 12],
        normal_force [N, 12] (lambda_n / h, newtons), friction_force [N, 12, 3] ((lambda_1 t_1 + lambda_2 t_2) / h, world frame),
        kind [N, 12] (0 ground, 1 wall plane, 2 maze box, 3 item cube, 4 self; -1 where not valid), item [N, 12] (cube index or -1),
        link, link2 [N, 12] int32 (level | leg << 2; link2 -1 unless a self contact), friction [N, 12] (the contact's coefficient),
        limit_impulse [N, 8] (signed, per joint), n_limit_rows, n_rows [N] int32, h [N].
    Slots beyond n hold zeros (kind / item / link2: -1)."""
    if raw.dim() != 2 or raw.shape[1] != K.HRL_CONTACTS_STRIDE:
        raise ValueError(f'contacts must be [N, {K.HRL_CONTACTS_STRIDE}], got {tuple(raw.shape)}')
    if cfg is not None and raw.shape[0] != cfg.num_envs:
        raise ValueError(f'contacts of {raw.shape[0]} envs, the config holds {cfg.num_envs}')
    c = raw[:, K.HRL_CONTACTS_HEADER:].unflatten(1, (K.HRL_CONTACT_MAX, K.HRL_CONTACT_WIDTH))
    n = raw[:, 0].to(torch.int32)
    valid = torch.arange(K.HRL_CONTACT_MAX, device=raw.device)[None, :] < n[:, None]
    h = raw[:, 3]
    inv_h = torch.where(h > 0, 1.0 / h, torch.zeros_like(h))[:, None]   # a record no step has written yet is all zeros
    surf, link, link2 = c[..., 16].to(torch.int32), c[..., 17].to(torch.int32), c[..., 18].to(torch.int32)
    is_self = valid & (link2 >= 0)
    is_item = valid & ~is_self & (surf >= K.HRL_SURF_ITEM)
    code = lambda v: torch.full_like(surf, v)   # (selects, not masked assignment: nothing here waits for the device)
    kind = torch.where(surf >= K.HRL_SURF_BOX, code(BOX), torch.where(surf >= 1, code(WALL), code(GROUND)))
    kind = torch.where(is_item, code(ITEM), torch.where(is_self, code(SELF), kind))
    kind = torch.where(valid, kind, code(-1))
    # the inverse of the kernel's surf_item(): cube i < 48 is HRL_SURF_ITEM + i, the cubes beyond sit behind the capsule-pair codes
    item = torch.where(is_item, torch.where(surf < K.HRL_SURF_SELF, surf - K.HRL_SURF_ITEM, surf - K.HRL_SURF_SELF), torch.full_like(surf, -1))
    return {'n': n, 'valid': valid, 'position': c[..., 0:3], 'distance': c[..., 3], 'normal': c[..., 4:7],
            'normal_force': c[..., 7] * inv_h,
            'friction_force': (c[..., 11:12] * c[..., 8:11] + c[..., 15:16] * c[..., 12:15]) * inv_h[:, :, None],
            'kind': kind, 'item': item, 'link': link, 'link2': torch.where(valid, link2, torch.full_like(link2, -1)),
            'friction': c[..., 19], 'limit_impulse': raw[:, 4:12],
            'n_limit_rows': raw[:, 1].to(torch.int32), 'n_rows': raw[:, 2].to(torch.int32), 'h': h}


def body_of_link(link):
    """Body index of a link code (level | leg << 2): 0 the torso (its sphere and the four jointless hip capsules, level 0), then per leg
    the aux body (1 + 2 leg) and the foot (2 + 2 leg)."""
    level, leg = link & 3, link >> 2
    return torch.where(level == 0, torch.zeros_like(link), 2 * leg + level)


def link_force(decoded):
    """[N, 9, 3]: the net external contact force on every body (torso, then per leg aux and foot) in the world frame -- what users of
    MuJoCo's `cfrc_ext` look for.  A self contact pushes its two bodies with equal and opposite forces; the point bot has body 0 only."""
    d = decoded
    f = (d['normal_force'][..., None] * d['normal'] + d['friction_force']) * d['valid'][..., None]
    out = torch.zeros(f.shape[0], 9, 3, dtype=f.dtype, device=f.device)
    out.scatter_add_(1, body_of_link(d['link']).long()[..., None].expand(-1, -1, 3), f)
    second = d['link2'] >= 0
    out.scatter_add_(1, body_of_link(d['link2'].clamp(min=0)).long()[..., None].expand(-1, -1, 3), -f * second[..., None])
    return out


KIND_NAMES = {GROUND: 'ground', WALL: 'wall', BOX: 'box', ITEM: 'item', SELF: 'self'}


def as_list(raw, index=0):
    """Env `index` of a raw tensor as a list of dicts of python numbers / tuples, one per contact, in the spirit of the tuples of pybullet's
    getContactPoints: position, normal, distance, normal_force, the two lateral friction forces with their directions, and what touches
    what (kind, item, link, link2)."""
    r = raw[index].detach().cpu()
    d = decode(r[None])
    h = float(r[3])
    out = []
    for i in range(int(d['n'][0])):
        c = r[K.HRL_CONTACTS_HEADER + K.HRL_CONTACT_WIDTH * i: K.HRL_CONTACTS_HEADER + K.HRL_CONTACT_WIDTH * (i + 1)].tolist()
        out.append({'position': tuple(c[0:3]), 'distance': c[3], 'normal': tuple(c[4:7]), 'normal_force': c[7] / h,
                    'lateral_friction1': c[11] / h, 'lateral_friction_dir1': tuple(c[8:11]),
                    'lateral_friction2': c[15] / h, 'lateral_friction_dir2': tuple(c[12:15]),
                    'kind': KIND_NAMES[int(d['kind'][0, i])], 'item': int(d['item'][0, i]), 'link': int(c[17]), 'link2': int(c[18]), 'friction': c[19]})
    return out
