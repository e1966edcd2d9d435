"""Test infrastructure only. CPU (PyTorch) restatement of the reference's aligned_aninerf_lbw eval render
(``aligned_aninerf_lbw_network.py:90-147`` under ``tpose_renderer.py:159-186``), op for op, on the helpers of
``oracle.restate`` / ``oracle.restate_sdf`` (KNN blend, embedders, LBS, weight norm, ``raw2outputs``). Runs in the
dtype of its inputs: float32 (pinned to the reference's fixtures G16 / G17 by tests/test_lbw_ref.py) or float64
(``to_dtype``; the neighbour search itself stays fp32, as in ``restate_sdf.sample_blend_closest_points``).

Weights: flat ``P`` dict with the reference state_dict names. Citations are into the reference tree.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import restate, restate_sdf

CHUNK = restate.CHUNK
NORM_TH = 0.05
FLOAT_KEYS = ('ray_o', 'ray_d', 'near', 'far', 'A', 'big_A', 'R', 'Th', 'pvertices', 'tvertices', 'weights', 'tbounds')


def to_dtype(P, batch, dtype):
    """(P, batch) with every floating tensor cast to ``dtype`` (tbounds becomes a private copy)."""
    P2 = {k: v.to(dtype) if v.is_floating_point() else v for k, v in P.items()}
    b2 = dict(batch)
    for k in FLOAT_KEYS:
        b2[k] = batch[k].to(dtype).clone()
    return P2, b2


def nerf_network(P, x):
    """NeRFNetwork.forward :336-352: gamma_6, 9 weight-normed layers, Softplus(beta=100), skip at 4 with /sqrt(2)."""
    inputs = restate.embed(x, 6)
    h = inputs
    for l in range(9):
        if l == 4:
            h = torch.cat([h, inputs], 1) / np.sqrt(2)
        h = restate_sdf._wn_linear(P, f'tpose_human.nerf_network.lin{l}', h)
        if l < 8:
            h = F.softplus(h, beta=100)
    return h


def color_network(P, points, view_dirs, feature, latent_index):
    """ColorNetwork.forward :403-436 (mode 'idr': points, gamma_4(view), feature; squeeze_out)."""
    x = torch.cat([points, restate.embed(view_dirs, 4), feature], dim=-1)
    pre = 'tpose_human.color_network.'
    net = F.relu(restate_sdf._wn_linear(P, pre + 'lin0', x))
    net = F.relu(restate_sdf._wn_linear(P, pre + 'lin1', net))
    net = F.relu(restate_sdf._wn_linear(P, pre + 'lin2', net))
    lat = F.embedding(latent_index, P[pre + 'color_latent.weight'])
    lat = lat.expand(net.size(0), lat.size(1))
    net = F.relu(restate_sdf._wn_linear(P, pre + 'lin3', torch.cat((net, lat), dim=1)))
    return torch.sigmoid(restate_sdf._wn_linear(P, pre + 'lin4', net))


def network_forward(P, wpts, viewdir, dists, batch, norm_th=NORM_TH, train_th=0.0, trace=None):
    """Network.forward :90-147 -> {'raw' (1,n,4), 'pbw' (1,m,24), 'tbw' (1,m,24)}; widens batch['tbounds'] in
    place. ``trace`` (dict) receives the intermediates G16 records."""
    wpts = wpts[None]
    pose_pts = restate.world_to_pose(wpts, batch['R'], batch['Th'])
    viewdir = viewdir[None]
    pose_dirs = restate_sdf.world_dirs_to_pose_dirs(viewdir, batch['R'])
    _, pnorm = restate_sdf.sample_blend_closest_points(pose_pts, batch['pvertices'], batch['weights'])
    pnorm = pnorm[..., 0]
    pind = pnorm < norm_th
    pind[torch.arange(len(pnorm)), pnorm.argmin(dim=1)] = True
    pose_pts = pose_pts[pind][None]
    pose_dirs = pose_dirs[pind][None]
    dists = dists[pind[0]]
    # pose_points_to_tpose_points :60-88
    init_pbw, _ = restate_sdf.sample_blend_closest_points(pose_pts, batch['pvertices'], batch['weights'])
    init_pbw = init_pbw.permute(0, 2, 1)
    pbw = restate.neural_blend_weights(P, pose_pts, init_pbw, batch['latent_index'] + 1)
    tpose = restate.lbs_to_tpose(pose_pts, pbw, batch['A'])
    tpose = restate_sdf.tpose_points_to_pose_points(tpose, pbw, batch['big_A'])
    init_tdirs = restate_sdf.pose_dirs_to_tpose_dirs(pose_dirs, pbw, batch['A'])
    tpose_dirs = restate_sdf.tpose_dirs_to_pose_dirs(init_tdirs, pbw, batch['big_A'])
    # T-pose blend weights :112-115
    init_tbw, _ = restate_sdf.sample_blend_closest_points(tpose, batch['tvertices'], batch['weights'])
    init_tbw = init_tbw.permute(0, 2, 1)
    tbw = restate.neural_blend_weights(P, tpose, init_tbw, torch.zeros_like(batch['latent_index']))
    tpose = tpose[0]
    vd = tpose_dirs[0]
    # TPoseHuman.forward :243-260
    out = nerf_network(P, tpose)
    dens = out[:, 0]
    alpha = 1. - torch.exp(-F.relu(dens) * dists)
    rgb = color_network(P, tpose, vd, out[:, 1:], batch['latent_index'])
    raw_c = torch.cat((rgb, alpha[:, None]), dim=1)
    th_raw = raw_c.clone()
    tbounds = batch['tbounds'][0]
    tbounds[0] -= 0.05
    tbounds[1] += 0.05
    inside = (tpose > tbounds[:1]) * (tpose < tbounds[1:])
    outside = torch.sum(inside, dim=1) != 3
    raw_c[outside] = 0
    alpha = raw_c[..., -1]
    raw = torch.zeros([1, wpts.shape[1], 4]).to(wpts)
    raw[pind] = raw_c
    alpha = alpha[None]
    alpha_ind = alpha > train_th
    alpha_ind[torch.arange(alpha.size(0)), torch.argmax(alpha, dim=1)] = True
    if trace is not None:
        trace.setdefault('chunks', []).append(dict(
            pnorm=pnorm, pind=pind, init_pbw=init_pbw.permute(0, 2, 1), init_tbw=init_tbw.permute(0, 2, 1), pbw=pbw,
            tbw=tbw, tpose=tpose, tpose_dirs=vd, th_raw=th_raw, density=dens, dists=dists, alpha_ind=alpha_ind[0],
            tbounds=tbounds.clone()))
    return {'raw': raw, 'pbw': pbw.transpose(1, 2)[alpha_ind][None], 'tbw': tbw.transpose(1, 2)[alpha_ind][None]}


def render_chunk(P, ray_o, ray_d, near, far, batch, t_rand=None, trace=None, **kw):
    """get_pixel_value, tpose_renderer.py:71-157."""
    pts, z = restate.sample_points(ray_o, ray_d, near, far, 64, t_rand)
    nb, npix, ns = pts.shape[:3]
    wpts = pts.view(nb * npix * ns, -1)
    vd = ray_d[:, :, None].repeat(1, 1, ns, 1).contiguous().view(nb * npix * ns, -1)
    dists = z[..., 1:] - z[..., :-1]
    dists = torch.cat([dists, dists[..., -1:]], dim=2).view(nb * npix * ns)
    ret = network_forward(P, wpts, vd, dists, batch, trace=trace, **kw)
    raw = ret['raw'].reshape(-1, ns, 4)
    rgb_map, acc, depth, _ = restate.raw2outputs(raw, z.view(-1, ns))
    return {'pbw': ret['pbw'].view(nb, -1, 24), 'tbw': ret['tbw'].view(nb, -1, 24),
            'rgb_map': rgb_map.view(nb, npix, -1), 'acc_map': acc.view(nb, npix),
            'depth_map': depth.view(nb, npix), 'raw': raw.view(nb, -1, 4)}


def render(P, batch, t_rand=None, chunk=CHUNK, trace=None, **kw):
    """Renderer.render, tpose_renderer.py:159-186 (mutates batch['tbounds']). ``t_rand`` (R, 64) or None."""
    R = batch['ray_o'].shape[1]
    outs = []
    with torch.no_grad():
        for i in range(0, R, chunk):
            tr = None if t_rand is None else t_rand[None, i:i + chunk]
            outs.append(render_chunk(P, batch['ray_o'][:, i:i + chunk], batch['ray_d'][:, i:i + chunk],
                                     batch['near'][:, i:i + chunk], batch['far'][:, i:i + chunk], batch,
                                     t_rand=tr, trace=trace, **kw))
    return {k: torch.cat([o[k] for o in outs], dim=1) for k in outs[0]}


# ---- fixtures ---------------------------------------------------------------------------------------------
def scene_batch(ray_o, ray_d, latent_index=7, shrink=0.0, rays=None):
    """(batch of torch tensors, P) for the synthetic PdfScene and the seeded lbw weights, over the rays that hit
    the box (``rays``: an index or slice into the hits); tbounds moved in by ``shrink`` per face as G17's."""
    from animatable_nerf_amd import synthetic
    import json
    import os
    scene = _scene()
    near, far, mask = restate.near_far(scene.pbounds, ray_o, ray_d)
    near, far = near.astype(np.float32), far.astype(np.float32)
    ro, rd = ray_o[mask], ray_d[mask]
    if rays is not None:
        ro, rd, near, far = ro[rays], rd[rays], near[rays], far[rays]
    b = scene.batch_arrays(ro, rd, near, far, latent_index=latent_index)
    b['tbounds'][0, 0] += np.float32(shrink)
    b['tbounds'][0, 1] -= np.float32(shrink)
    batch = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in b.items()}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_state_dict.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    P = {k: torch.from_numpy(v) for k, v in synthetic.init_state_dict_lbw(shapes).items()}
    return batch, P


_SCENE = []


def _scene():
    if not _SCENE:
        from animatable_nerf_amd.synthetic import PdfScene
        _SCENE.append(PdfScene(vsize=0.05))
    return _SCENE[0]


def lbw_cfg(**overrides):
    from animatable_nerf_amd import config
    return config.subject('aligned_aninerf_lbw_s9p', perturb=0, **overrides)


def make_net(P, device='cpu', cfg=None):
    """network_lbw.Network holding the weights P (reference state_dict names)."""
    from animatable_nerf_amd import network_lbw
    net = network_lbw.Network(cfg if cfg is not None else lbw_cfg())
    net.load_state_dict({k: v.clone() for k, v in P.items()}, strict=True)
    return net.to(device)


EDGE_MARGIN = 1e-4  # the project's fp32 tolerance (tests/test_gpu_sdf.py TOL)


def edge_samples(trace, margin=EDGE_MARGIN):
    """Sample ids (ray * 64 + sample, over the whole frame) whose ``alpha > 0`` decision sits on an fp32 edge,
    from a float64 run's trace: the density is within ``margin`` of 0, or the warped point is within ``margin``
    of a face of its chunk's widened box. A path whose values are within ``margin`` of the exact ones can decide
    such a sample either way, and no other."""
    out, base = [], 0
    for c in trace['chunks']:
        ids = torch.nonzero(c['pind'][0])[:, 0] + base
        tb = c['tbounds']
        near_face = ((c['tpose'] - tb[:1]).abs().min(dim=1)[0] < margin) | ((c['tpose'] - tb[1:]).abs().min(dim=1)[0] < margin)
        edge = (c['density'].abs() < margin) | near_face
        out.append(ids[edge])
        base += c['pind'].shape[1]
    return torch.cat(out).numpy().astype(np.int64)
