"""Host-side helpers with the reference's names (reference utils.py:615-682 for the training path, 825-865 and 1405-1412 for the test phase,
773-781 and 1246-1295 for the test output in the tracker's frame, 1462-1482 and 1734-1744 for teacher-student training)."""

import torch


def kaiming_weight_zero_bias(model, mode="fan_in", activation_mode="relu", distribution="uniform"):
    """reference utils.py:655-671: Kaiming init of every non-BN weight, BN weight = 1, biases 0."""
    if activation_mode == "leaky_relu":
        raise ValueError("Leaky relu is not supported yet")
    with torch.no_grad():
        for module in model.modules():
            weight = getattr(module, "weight", None)
            if isinstance(weight, torch.Tensor):
                if 'BatchNorm' not in module.__class__.__name__:
                    init = torch.nn.init.kaiming_uniform_ if distribution == "uniform" else torch.nn.init.kaiming_normal_
                    init(weight, mode=mode, nonlinearity=activation_mode)
                else:
                    weight.fill_(1)
            bias = getattr(module, "bias", None)
            if isinstance(bias, torch.Tensor):
                bias.zero_()


def init_net(net, type="kaiming", mode="fan_in", activation_mode="relu", distribution="normal"):
    """reference utils.py:619-626 (called train.py:193): move to the GPU and initialise."""
    if not torch.cuda.is_available():
        raise RuntimeError("init_net needs a HIP device (reference utils.py:620 asserts the same)")
    net = net.cuda()
    if type != "kaiming":
        raise ValueError("only the Kaiming initialisation used by train.py is provided")
    kaiming_weight_zero_bias(net, mode=mode, activation_mode=activation_mode, distribution=distribution)
    return net


def generating_pos_and_increment(idx, visible_view_indexes, adjacent_range, rng=None):
    """reference utils.py:412-438 (called dataset.py:346-350): position of the first frame of a training pair inside the
    sequence's visible views and the signed gap to its partner, drawn from ``adjacent_range`` = (min gap, max gap) -- the
    "adjacent range 5-30" of BASELINE.json configs[4].  Host-side pair selection: it consumes Python's ``random`` exactly as the
    reference does (same calls in the same order), so a seeded run picks the same pairs.  ``rng``: a ``random.Random`` to draw
    from instead of the module-level generator (same calls; lets an iterator own its seed -- dataset.TrainingBatches)."""
    import random
    if rng is not None:
        random = rng
    visible_view_idx = idx % len(visible_view_indexes)
    low, high = adjacent_range[0], adjacent_range[1]
    count = len(visible_view_indexes)
    if count <= 2 * low:
        low = count // 2
    if visible_view_idx <= low - 1:
        increment = random.randint(low, min(high, count - 1 - visible_view_idx))
    elif visible_view_idx >= count - low:
        increment = -random.randint(low, min(high, visible_view_idx))
    else:
        if random.randint(0, 1) == 1:
            increment = random.randint(low, min(high, count - 1 - visible_view_idx))
        else:
            increment = -random.randint(low, min(high, visible_view_idx))
    return [visible_view_idx, increment]


def save_model(model, optimizer, epoch, step, model_path, validation_loss, module_prefix=True):
    """reference utils.py:674-682 wire format {model, optimizer, epoch, step, validation}; keys carry
    the 'module.' prefix the reference's DataParallel wrapper adds (train.py:197)."""
    state = model.state_dict()
    if module_prefix:
        state = {"module." + k: v for k, v in state.items()}
    torch.save({'model': state, 'optimizer': optimizer.state_dict(), 'epoch': epoch, 'step': step,
                'validation': validation_loss}, str(model_path))


def load_checkpoint(model_path, model=None, optimizer=None, map_location=None):
    """Read a checkpoint file in the reference's wire format (utils.py:674-682) and, when given, restore ``model`` (keys with or
    without 'module.', train.py:222 / evaluate.py:150) and ``optimizer`` (torch.optim.SGD's layout: FusedClipSGD or SGD).  Returns
    the dictionary {model, optimizer, epoch, step, validation}.  The file is a pickle and is read as one (the param group's lr is a
    numpy scalar once scheduler.CyclicLR has stepped, which torch's weights-only loader refuses): load files you trust, exactly as
    the reference's own ``torch.load(path)`` (train.py:218) assumes."""
    state = torch.load(str(model_path), map_location=map_location, weights_only=False)
    if model is not None:
        load_model_state(model, state["model"])
    if optimizer is not None:
        optimizer.load_state_dict(state["optimizer"])
    return state


def load_model_state(model, state):
    """Load a reference checkpoint's ``state['model']`` with or without the 'module.' prefix."""
    cleaned = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}
    return model.load_state_dict(cleaned)


def point_cloud_from_depth(depth_map, color_img, mask_img, intrinsic_matrix, point_cloud_downsampling,
                           min_threshold=None, max_threshold=None, device="cuda"):
    """Drop-in for reference utils.py:823-852 on the GPU (endo_point_cloud): (P, 6) float32 numpy array of
    (x, y, z, r, g, b), row-major over the kept pixels.  The reference walks 81 920 pixels in a Python double loop per
    frame (evaluate.py:272,340); this is three small kernels.  Inputs may be numpy arrays or tensors (any device);
    there is no CPU fallback."""
    import numpy as np
    from . import _lib
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("point_cloud_from_depth needs a GPU device: the MI355X path has no CPU fallback")
    depth = torch.as_tensor(np.asarray(depth_map.detach().cpu() if torch.is_tensor(depth_map) else depth_map), dtype=torch.float32)
    height, width = int(depth.shape[0]), int(depth.shape[1])
    depth = depth.contiguous().to(dev)
    color = torch.as_tensor(np.ascontiguousarray(np.asarray(color_img.detach().cpu() if torch.is_tensor(color_img) else color_img)
                                                 .reshape(height, width, 3)).astype(np.uint8)).to(dev)
    mask = torch.as_tensor(np.asarray(mask_img.detach().cpu() if torch.is_tensor(mask_img) else mask_img), dtype=torch.float32)
    mask = mask.reshape(height, width).contiguous().to(dev)
    k = torch.as_tensor(np.asarray(intrinsic_matrix.detach().cpu() if torch.is_tensor(intrinsic_matrix) else intrinsic_matrix),
                        dtype=torch.float32).reshape(3, 3).contiguous().to(dev)
    use_thr = max_threshold is not None and min_threshold is not None
    points = torch.empty((height * width, 6), dtype=torch.float32, device=dev)
    offsets = torch.empty(height + 1, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.endo_point_cloud(_lib.ptr(depth), _lib.ptr(color), _lib.ptr(mask), _lib.ptr(k), height, width,
                                  int(point_cloud_downsampling), 1 if use_thr else 0,
                                  float(min_threshold) if use_thr else 0.0, float(max_threshold) if use_thr else 0.0,
                                  _lib.ptr(offsets), _lib.ptr(points), _lib.ptr(count), _lib.stream())
    _lib.check(rc, "endo_point_cloud")
    n = int(count.item())
    return points[:n].cpu().numpy().reshape(-1, 6)


def _host_f32(x, shape):
    import numpy as np
    return np.ascontiguousarray(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x), dtype=np.float32).reshape(shape)


def _colors_from_u8(color_img, height, width):
    """(1, 3, H, W) float32 colours c with uint8(255 * clip(0.5 c + 0.5, 0, 1)) == color_img exactly: c = (u + 0.5) / 127.5 - 1 puts
    255 * (0.5 c + 0.5) at u + 0.5, half a unit from both truncation edges (u = 255: clipped to 1)."""
    import numpy as np
    u = np.asarray(color_img.detach().cpu() if torch.is_tensor(color_img) else color_img).reshape(height, width, 3).astype(np.uint8)
    c = (u.astype(np.float32) + np.float32(0.5)) / np.float32(127.5) - np.float32(1.0)
    return np.ascontiguousarray(c.transpose(2, 0, 1).reshape(1, 3, height, width), dtype=np.float32)


def point_cloud_from_depth_and_initial_pose(depth_map, color_img, mask_img, intrinsic_matrix, translation, rotation,
                                            point_cloud_downsampling, min_threshold=None, max_threshold=None, device="cuda"):
    """Drop-in for reference utils.py:1246-1295 on the GPU (endo_evaluate_posed on one frame): (P, 6) float32 numpy array of
    (x, y, z, r, g, b) over the kept pixels in row-major order, the cloud normalised to a z range of 20 units and moved into the
    tracker's frame by ``rotation`` (3, 3) and ``translation`` (3,), float64.  As in the reference, (r, g, b) are channels (2, 1, 0) of
    ``color_img`` (H, W, 3) uint8, the z range is that of the kept pixels whether or not the thresholds write them, and a mask
    without kept pixels raises ZeroDivisionError (the reference's z_min / z_max sentinels are Python ints).  The arithmetic is the
    reference's under numpy 2 (a float32 scale).  Inputs may be numpy arrays or tensors (any device); there is no CPU fallback."""
    import numpy as np
    from . import evaluate
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("point_cloud_from_depth_and_initial_pose needs a GPU device: the MI355X path has no CPU fallback")
    shape = np.asarray(color_img.detach().cpu() if torch.is_tensor(color_img) else color_img).shape
    height, width = int(shape[0]), int(shape[1])
    depth = torch.from_numpy(_host_f32(depth_map, (1, 1, height, width))).to(dev)
    mask = torch.from_numpy(_host_f32(mask_img, (1, 1, height, width))).to(dev)
    k = torch.from_numpy(_host_f32(intrinsic_matrix, (1, 3, 3))).to(dev)
    colors = torch.from_numpy(_colors_from_u8(color_img, height, width)).to(dev)
    # the entry forms d = boundary * prediction: with the {0, 1}-valued mask as the boundary every kept pixel's d is depth_map's value
    kept_mask = (mask > 0.5).to(torch.float32)
    out = evaluate.posed_outputs_from_predictions(colors, kept_mask, depth, k, np.asarray(rotation, np.float64).reshape(1, 3, 3),
                                                  np.asarray(translation, np.float64).reshape(1, 3), False, int(point_cloud_downsampling),
                                                  min_threshold, max_threshold)
    if out["ranges"][0, 0] > out["ranges"][0, 1]:
        raise ZeroDivisionError("float division by zero")
    return out["points"][:out["offsets"][1]].cpu().numpy().reshape(-1, 6)


def display_depth_map(depth_map, min_value=None, max_value=None, device="cuda"):
    """Drop-in for reference utils.py:773-781 with COLORMAP_JET on the GPU (endo_evaluate_posed's depth image of one frame): (H, W, 3)
    uint8 B, G, R of COLORMAP_JET[uint8(|(d - min) / (max - min) * 255|)] with the map's own minimum and maximum.  A constant map
    (0 / 0 in the reference) takes entry 0 everywhere.  The device entry takes the range from the map itself, which is what every call
    in the reference does; explicit min_value / max_value raise NotImplementedError."""
    import numpy as np
    from . import evaluate
    if min_value is not None and max_value is not None:
        raise NotImplementedError("display_depth_map with an explicit range: endo_evaluate_posed takes each map's own minimum and maximum")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("display_depth_map needs a GPU device: the MI355X path has no CPU fallback")
    d = np.asarray(depth_map.detach().cpu() if torch.is_tensor(depth_map) else depth_map, dtype=np.float32)
    d = d.reshape(d.shape[0], d.shape[1])
    height, width = d.shape
    depth = torch.from_numpy(np.ascontiguousarray(d).reshape(1, 1, height, width)).to(dev)
    ones = torch.ones((1, 1, height, width), dtype=torch.float32, device=dev)
    zeros = torch.zeros((1, 3, height, width), dtype=torch.float32, device=dev)
    k = torch.eye(3, dtype=torch.float32, device=dev).reshape(1, 3, 3)
    out = evaluate.posed_outputs_from_predictions(zeros, ones, depth, k, np.eye(3).reshape(1, 3, 3), np.zeros((1, 3)))
    return out["depth_images"][0].cpu().numpy()


class _DistillFn(torch.autograd.Function):
    """0.5 * (ScaleInvariantLoss(|p1|, |g1|, b) + ScaleInvariantLoss(|p2|, |g2|, b)) on the packed (2N, 1, H, W) predictions as one
    node: endo_distill_head computes value and d / d prediction together, the backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, pred, goal, boundaries, eps):
        from . import _lib, train_step
        pred = _lib.dev_f32(pred, "predictions")
        goal = _lib.dev_f32(goal, "goals")
        boundaries = _lib.dev_f32(boundaries, "boundaries")
        if pred.dim() != 4 or pred.shape[1] != 1 or pred.shape[0] % 2 or goal.shape != pred.shape:
            raise ValueError("expected (2N, 1, H, W) predictions and goals (got %s and %s)" % (tuple(pred.shape), tuple(goal.shape)))
        if tuple(boundaries.shape) != (pred.shape[0] // 2, 1) + tuple(pred.shape[2:]):
            raise ValueError("expected (N, 1, H, W) boundaries (got %s)" % (tuple(boundaries.shape),))
        losses_t = torch.empty(5, dtype=torch.float32, device=pred.device)
        grad_pred = torch.empty_like(pred)
        train_step._distill_head(pred, goal, boundaries, 1.0, float(eps), False, losses_t, grad_pred)
        ctx.save_for_backward(grad_pred)
        return losses_t[4].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise RuntimeError("learn_from_teacher: the teacher's depths and the boundaries get no gradient")
        (grad_pred,) = ctx.saved_tensors
        return grad_pred * grad_loss, None, None, None


def _forward_pair(model, x1, x2):
    if hasattr(model, "forward_pair_packed"):
        return model.forward_pair_packed(x1, x2)
    return torch.cat([model(x1), model(x2)], dim=0)


def learn_from_teacher(boundaries, colors_1, colors_2, depth_estimation_model_teacher, depth_estimation_model_student,
                       scale_invariant_loss):
    """reference utils.py:1462-1482 for callers who keep their own loop: the teacher-student loss of one frame pair,
    ``0.5 * (SIL(|student(c1)|, |teacher(c1)|, b) + SIL(|student(c2)|, |teacher(c2)|, b))``, differentiable with respect to the
    student's parameters (one autograd node over endo_distill_head, then the student's), and the four absolute depth maps.  The teacher
    runs under ``no_grad`` in its current mode; eps is ``scale_invariant_loss.epsilon`` (losses.ScaleInvariantLoss).  The returned maps
    are the network outputs themselves when the models are FCDenseNets, whose last operation is already ``torch.abs`` (models.py:186).
    ``train_step.DistillationStep`` is the fused iteration around the same head."""
    with torch.no_grad():
        goal = _forward_pair(depth_estimation_model_teacher, colors_1, colors_2)
    pred = _forward_pair(depth_estimation_model_student, colors_1, colors_2)
    loss = _DistillFn.apply(pred, goal, boundaries, scale_invariant_loss.epsilon)
    n = pred.shape[0] // 2
    outputs = (pred[:n], pred[n:], goal[:n], goal[n:])
    if not (hasattr(depth_estimation_model_teacher, "forward_pair_packed") and hasattr(depth_estimation_model_student, "forward_pair_packed")):
        outputs = tuple(torch.abs(t) for t in outputs)
    return (loss,) + outputs


def calculate_outlier_robust_validation_loss(validation_losses, previous_validation_losses):
    """reference utils.py:1734-1744, the model-selection criterion of the teacher-student loop: for per-sample loss arrays of equal
    length, (number of increases) * (sum of increases) + (number of decreases) * (sum of decreases, negative); -1.0 when the new
    array is longer, 1.0 when it is shorter.  Host numpy."""
    import numpy as np
    if len(validation_losses) == len(previous_validation_losses):
        differences = np.asarray(validation_losses) - np.asarray(previous_validation_losses)
        up, down = differences > 0.0, differences < 0.0
        positive = np.sum(np.sum(np.int32(up)) * up * differences)
        negative = np.sum(np.sum(np.int32(down)) * down * differences)
        return positive + negative
    return -1.0 if len(validation_losses) > len(previous_validation_losses) else 1.0


def get_filenames_from_frame_indexes(sequence_root, frame_index_array):
    """reference utils.py:1405-1412 (evaluate.py --load_all_frames, with reader.read_visible_view_indexes): the ``%08d.jpg`` file of
    every frame index found anywhere below ``sequence_root``, missing frames skipped, the list sorted.  A frame found in several
    subfolders gives the first of them in sorted order (the reference takes the first ``rglob`` yields, which is file-system order)."""
    import pathlib
    root = pathlib.Path(sequence_root)
    names = []
    for index in frame_index_array:
        found = sorted(root.rglob("{:08d}.jpg".format(int(index))))
        if found:
            names.append(found[0])
    names.sort()
    return names


_PLY_PROPERTIES = ("property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                   "property uchar blue")


def write_point_cloud(path, point_cloud, text=True):
    """reference utils.py:855-865 without plyfile: one ``vertex`` element of float x, y, z and uchar red, green, blue per row of the
    (P, 6) float32 array -- what ``PlyData([el], text=True).write(path)`` stores.  text=True: ASCII PLY 1.0, one vertex per line, the
    floats with 9 significant digits (every float32 reads back exactly); text=False: binary_little_endian 1.0."""
    import numpy as np
    points = np.asarray(point_cloud, dtype=np.float32).reshape(-1, 6)
    n = points.shape[0]
    header = "\n".join(("ply", "format ascii 1.0" if text else "format binary_little_endian 1.0", "element vertex %d" % n)
                       + _PLY_PROPERTIES + ("end_header",)) + "\n"
    with open(str(path), "wb") as f:
        f.write(header.encode("ascii"))
        if text:
            if n:
                # the colours print as integers: plyfile casts them to uchar first (utils.py:862), these are whole numbers in [0, 255]
                f.write((("%.9g %.9g %.9g %d %d %d\n" * n) % tuple(points.astype(np.float64).ravel().tolist())).encode("ascii"))
        else:
            rec = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
            for k, name in enumerate(("x", "y", "z", "red", "green", "blue")):
                rec[name] = points[:, k]
            f.write(rec.tobytes())


_PLY_MESH_PROPERTIES = ("property float x", "property float y", "property float z", "property float nx", "property float ny",
                        "property float nz", "property uchar red", "property uchar green", "property uchar blue")


def write_mesh(path, vertices, normals, faces, text=False):
    """A triangle mesh as PLY 1.0 without plyfile: a ``vertex`` element of float x, y, z, float nx, ny, nz and uchar red, green, blue
    from the (P, 6) float32 ``vertices`` (x, y, z, r, g, b: fusion.TSDFVolume.extract_mesh's, the colours whole numbers in
    [0, 255]) and the (P, 3) float32 ``normals``, and a ``face`` element of ``property list uchar int vertex_indices`` from the
    (T, 3) int32 ``faces``.  text=False: binary_little_endian; text=True: ASCII in write_point_cloud's number format, one vertex or
    face per line.  P = 0 and T = 0 are valid."""
    import numpy as np
    points = np.asarray(vertices, dtype=np.float32).reshape(-1, 6)
    normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    n, t = points.shape[0], faces.shape[0]
    if normals.shape[0] != n:
        raise ValueError("write_mesh expects one normal per vertex: %d normals for %d vertices" % (normals.shape[0], n))
    if t and (faces.min() < 0 or faces.max() >= n):
        raise ValueError("write_mesh: a face index lies outside the %d vertices" % n)
    header = "\n".join(("ply", "format ascii 1.0" if text else "format binary_little_endian 1.0", "element vertex %d" % n)
                       + _PLY_MESH_PROPERTIES + ("element face %d" % t, "property list uchar int vertex_indices", "end_header")) + "\n"
    with open(str(path), "wb") as f:
        f.write(header.encode("ascii"))
        if text:
            if n:
                both = np.concatenate([points[:, :3], normals, points[:, 3:]], axis=1).astype(np.float64)
                f.write((("%.9g %.9g %.9g %.9g %.9g %.9g %d %d %d\n" * n) % tuple(both.ravel().tolist())).encode("ascii"))
            if t:
                f.write((("3 %d %d %d\n" * t) % tuple(faces.ravel().tolist())).encode("ascii"))
        else:
            rec = np.empty(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                     ("red", "u1"), ("green", "u1"), ("blue", "u1")])
            for k, name in enumerate(("x", "y", "z")):
                rec[name] = points[:, k]
                rec["n" + name] = normals[:, k]
            for k, name in enumerate(("red", "green", "blue")):
                rec[name] = points[:, 3 + k]
            f.write(rec.tobytes())
            tri = np.empty(t, dtype=[("count", "u1"), ("index", "<i4", (3,))])
            tri["count"] = 3
            tri["index"] = faces
            f.write(tri.tobytes())


def write_png(path, bgr, compress_level=1):
    """cv2.imwrite(path, bgr) for an (H, W, 3) uint8 image in cv2's B, G, R order, with zlib and struct only: an 8-bit RGB PNG
    (colour type 2, no interlace, filter type 0 on every row).  The pixels are the contract, not libpng's bytes."""
    import struct
    import zlib
    import numpy as np
    img = np.asarray(bgr)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("write_png expects an (H, W, 3) uint8 array")
    height, width = img.shape[:2]
    raw = np.zeros((height, 1 + 3 * width), dtype=np.uint8)          # a filter-type byte (0) in front of each row
    raw[:, 1:] = img[:, :, ::-1].reshape(height, 3 * width)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    with open(str(path), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw.tobytes(), compress_level)))
        f.write(chunk(b"IEND", b""))
