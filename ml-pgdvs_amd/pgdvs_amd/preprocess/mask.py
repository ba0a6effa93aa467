"""The ``flow_epi`` motion mask (pgdvs/preprocess/compute_mask.py:160-181 skew / compute_epipolar_distance, :196-215
read_optical_flow, :218-338 compute_mask_epipolar_flow): the epipolar distance of every pixel's flow correspondence, gated
by flow consistency, thresholded and opened with ``disk(1)``."""
import pathlib

import numpy as np

DISK1 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)  # skimage.morphology.disk(1)


def skew(x):
    return np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])


def fundamental_matrix(T_12, K_1, K_2):
    """F[3,3] float64 with l_2 = F p_1 (compute_mask.py:165-173): inv(K_2)^T [t_12]x R_12 inv(K_1), upstream's product order"""
    T_12, K_1, K_2 = (np.asarray(a, dtype=np.float64) for a in (T_12, K_1, K_2))
    E_mat = np.dot(skew(T_12[:3, 3]), T_12[:3, :3])
    return np.dot(np.dot(np.linalg.inv(K_2).T, E_mat), np.linalg.inv(K_1))


def binary_opening_disk1(raw):
    """skimage.morphology.binary_opening(raw, disk(1)) restated with scipy.ndimage: the erosion sees set pixels outside the
    image, the dilation clear ones"""
    from scipy import ndimage as ndi

    eroded = ndi.binary_erosion(raw, structure=DISK1, border_value=True)
    return ndi.binary_dilation(eroded, structure=DISK1, border_value=0)


def masked_epipolar_distance_numpy(flow, coord_diff, F, consist_thres=1.0):
    """e_dist[H,W] float64 of one direction (compute_mask.py:175-179, :213, :311-318, :330-332): p_2 = p + flow in float32,
    widened; |p_2 . F p| / (sqrt(l_0^2 + l_1^2) + 1e-8) in float64; times (sum|coord_diff| <= consist_thres)"""
    H, W = flow.shape[:2]
    xv, yv = np.meshgrid(range(0, W), range(0, H), indexing="xy")
    p_ref = np.float32(np.stack((xv, yv), axis=-1))
    ones = np.ones((H * W, 1))
    p_1 = np.concatenate((np.reshape(p_ref, (-1, 2)), ones), axis=-1).T
    p_2 = np.concatenate((np.reshape(p_ref + flow, (-1, 2)), ones), axis=-1).T
    l_2 = np.dot(F, p_1)
    n_term = np.sqrt(l_2[0, :] ** 2 + l_2[1, :] ** 2) + 1e-8
    e_dist = np.reshape(np.abs(np.sum(p_2 * l_2, axis=0) / n_term), (H, W))
    return e_dist * (np.sum(np.abs(coord_diff), axis=2) <= consist_thres)


def choose_direction(idx_ref, n_all_frames, all_w2c, flow_interval=1):
    """True: the mask of frame ``idx_ref`` comes from the flow to the PREVIOUS frame (compute_mask.py:243-306).  The first
    ``flow_interval`` frames have only a next frame, the last ones only a previous one; in between the neighbour whose
    camera centre is nearer in L1 decides, and a tie goes to the next frame."""
    if idx_ref < flow_interval:
        return False
    if idx_ref >= n_all_frames - flow_interval:
        return True
    centre = [np.linalg.inv(all_w2c[i])[:3, 3] for i in (idx_ref - flow_interval, idx_ref, idx_ref + flow_interval)]
    dist_ref_prev = np.sum(np.abs(centre[0] - centre[1]))
    dist_ref_post = np.sum(np.abs(centre[2] - centre[1]))
    return bool(dist_ref_prev < dist_ref_post)


def epipolar_motion_mask(idx_ref, n_all_frames, all_w2c, all_K, flow_dir, all_img_names, flow_interval=1, threshold=1.0,
                         device=None):
    """compute_mask_epipolar_flow's motion mask of frame ``idx_ref`` as bool [H,W], from the ``.npz`` of the chosen
    direction in ``flow_dir`` (an ``interval_<flow_interval>`` directory) alone: upstream computes both directions and keeps
    one.  ``device=None``: numpy and scipy.ndimage on the host; otherwise one HIP launch on ``device``
    (``ops.epipolar_mask``)."""
    all_w2c, all_K = np.asarray(all_w2c), np.asarray(all_K)
    use_prev = choose_direction(idx_ref, n_all_frames, all_w2c, flow_interval)
    idx_other = idx_ref - flow_interval if use_prev else idx_ref + flow_interval
    info = np.load(pathlib.Path(flow_dir) / f"{all_img_names[idx_ref]}_{all_img_names[idx_other]}.npz")
    flow, coord_diff = info["flow"], info["coord_diff"]
    T_ref2other = np.dot(all_w2c[idx_other], np.linalg.inv(all_w2c[idx_ref]))
    F = fundamental_matrix(T_ref2other, all_K[idx_ref], all_K[idx_other])
    if device is None:
        return binary_opening_disk1(masked_epipolar_distance_numpy(flow, coord_diff, F) > threshold)
    import torch

    from .. import ops

    mask = ops.epipolar_mask(torch.from_numpy(np.ascontiguousarray(flow, np.float32)).to(device),
                             torch.from_numpy(np.ascontiguousarray(coord_diff, np.float32)).to(device), F, threshold=threshold)
    return mask.cpu().numpy().astype(bool)
