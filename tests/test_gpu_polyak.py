"""polyak_ (ctr_polyak: the soft target update and the blob refresh in one launch) against a numpy
restatement of torch's lerp formula in float32, bit for bit: the target tensors afterwards, and the
blobs, which are ctr_actor_pack / ctr_critic_pack of the restatement's new targets, every byte.  The
shapes are the packer's (tests/test_gpu_actor_load.py) and the critic's two row lengths; tensors
carved out of one buffer with sentinels between them show every store in bounds; several nets share
one launch; special values, tau = 0 and tau = 1, graph capture, and torch's own lerp_ within a
derived bound."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (kind, hidden, in_dim): 6 -> 32 row padding, 19 -> 32 column padding; the tile count changes between
# layers; 16 k-steps and 8 tiles; close under the LDS budget; the critic's k-step 1 of layer 0
# reaches features 24 and 25
SHAPES = [("actor", (32,), 19), ("actor", (64, 96), 20), ("actor", (32, 256, 32), 20), ("actor", (224, 160), 19),
          ("critic", (32,), 25), ("critic", (64, 96), 26)]
CASES = [(k, h, d, tau) for k, h, d in SHAPES for tau in (0.001, 0.75) if not (h == (32, 256, 32) and tau == 0.75)]
SENTINEL = np.uint32(0x4B3C2D1E)
GAP = 8


def _reference(t, p, tau):
    """torch's lerp formula, every operation a float32 numpy operation (one rounding each)."""
    tau32 = np.float32(tau)
    with np.errstate(all="ignore"):
        d = p - t
        if tau32 < 0.5:
            r = t + tau32 * d
        else:
            r = p - d * (np.float32(1) - tau32)
    assert r.dtype == np.float32
    return r


def _layers(rng, kind, hidden, in_dim, scale=None):
    """U(+-1/sqrt(fan_in)) weights and biases (``scale``: U(+-scale) instead), numpy float32."""
    dims = [in_dim] + list(hidden) + [6 if kind == "actor" else 1]
    layers = []
    for l in range(len(dims) - 1):
        s = scale or 1.0 / np.sqrt(dims[l])
        layers.append((rng.uniform(-s, s, (dims[l + 1], dims[l])).astype(np.float32),
                       rng.uniform(-s, s, dims[l + 1]).astype(np.float32)))
    return layers


def _net(kind, layers, cuda):
    from ctr_reach_amd.policy import MlpActor, MlpCritic
    if kind == "actor":
        return MlpActor(layers, np.array([0.001, 0.001, 0.001, 0.087, 0.087, 0.087]), device=cuda)
    return MlpCritic(layers, device=cuda)


def _host_pack(net, layers):
    """ctr_actor_pack / ctr_critic_pack of ``layers`` (numpy) into a host buffer prefilled with 0xAB."""
    from ctr_reach_amd import _abi
    lib = _abi.load()
    nb = getattr(lib, "ctr_%s_blob_bytes" % net.NAME)(net._struct)
    out = np.full(nb, 0xAB, dtype=np.uint8)
    n = len(layers)
    keep = [(np.ascontiguousarray(w), np.ascontiguousarray(v)) for w, v in layers]
    W = (ctypes.c_void_p * n)(*[w.ctypes.data for w, _ in keep])
    b = (ctypes.c_void_p * n)(*[v.ctypes.data for _, v in keep])
    assert getattr(lib, "ctr_%s_pack" % net.NAME)(net._struct, W, b, out.ctypes.data) == 0
    return out


def _device(layers, cuda):
    import torch
    return [(torch.from_numpy(W.copy()).to(cuda), torch.from_numpy(b.copy()).to(cuda)) for W, b in layers]


def _host(dev):
    return [(W.cpu().numpy(), b.cpu().numpy()) for W, b in dev]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _step(online, target, tau):
    """The restatement's new targets, layer by layer."""
    return [(_reference(Wt, W, tau), _reference(bt, b, tau)) for (W, b), (Wt, bt) in zip(online, target)]


def _assert_targets(got, want, tag):
    """Bit for bit; where the restatement gives NaN, any NaN (payload propagation is not specified).
    Returns ``want`` with the device's NaNs, the values the blob was packed from."""
    out = []
    for l, (gl, wl) in enumerate(zip(got, want)):
        pair = []
        for name, g, w in zip("Wb", gl, wl):
            assert g.shape == w.shape and g.dtype == np.float32
            nan = np.isnan(w)
            assert np.isnan(g[nan]).all(), (tag, l, name, "NaN expected")
            bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(-1) & ~nan.reshape(-1))
            assert bad.size == 0, (tag, l, name, bad.size, bad[:8].tolist(), g.reshape(-1)[bad[:8]].tolist(),
                                   w.reshape(-1)[bad[:8]].tolist())
            pair.append(np.where(nan, g, w))
        out.append(tuple(pair))
    return out


def _assert_blob(net, layers, tag):
    import torch
    torch.cuda.synchronize()
    got, want = net.blob.cpu().numpy(), _host_pack(net, layers)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _assert_unchanged(dev, before, tag):
    for l, ((W, b), (W0, b0)) in enumerate(zip(_host(dev), before)):
        assert np.array_equal(_bits(W), _bits(W0)) and np.array_equal(_bits(b), _bits(b0)), (tag, l)


@pytest.mark.parametrize("kind,hidden,in_dim,tau", CASES)
def test_one_net_is_the_restatement_bit_for_bit(cuda, kind, hidden, in_dim, tau):
    rng = np.random.default_rng(100 + len(hidden) + in_dim)
    online, target = _layers(rng, kind, hidden, in_dim), _layers(rng, kind, hidden, in_dim)
    net = _net(kind, _layers(rng, kind, hidden, in_dim), cuda)
    net.blob.fill_(0xAB)                                 # the kernel must not rely on zeroed padding
    ptr = net.blob.data_ptr()
    d_on, d_tg = _device(online, cuda), _device(target, cuda)
    assert net.polyak_(d_on, d_tg, tau) is net
    want = _assert_targets(_host(d_tg), _step(online, target, tau), (kind, hidden, in_dim, tau))
    _assert_unchanged(d_on, online, "online")
    _assert_blob(net, want, (kind, hidden, in_dim, tau))
    assert net.blob.data_ptr() == ptr == net._struct.blob                # in place
    assert net.weights is None and net.biases is None and net.packed is None
    assert all(a.data_ptr() == b.data_ptr() for pair, src in zip(d_tg, net._sources) for a, b in zip(pair, src))
    # (the update moved the targets, and by tau of the way)
    assert not np.array_equal(want[0][0], target[0][0]) and not np.array_equal(want[0][0], online[0][0])


def _carve(layers, cuda):
    """``layers`` as contiguous views into one flat device buffer that starts them at float offset 1
    and leaves GAP sentinel floats between them: (views [(W, b), ...], the buffer, the mask of the
    sentinel floats)."""
    import torch
    sizes = [a.size for pair in layers for a in pair]
    flat = np.full(1 + sum(sizes) + GAP * len(sizes), SENTINEL, dtype=np.uint32)
    guard = np.ones(flat.size, dtype=bool)
    spans, off = [], 1
    for pair in layers:
        for a in pair:
            flat[off:off + a.size] = _bits(a).reshape(-1)
            guard[off:off + a.size] = False
            spans.append((off, a.shape))
            off += a.size + GAP
    buf = torch.from_numpy(flat.view(np.float32)).to(cuda)
    views = [buf[o:o + int(np.prod(shape))].view(*shape) for o, shape in spans]
    assert all(v.is_contiguous() and v.data_ptr() == buf.data_ptr() + 4 * o for v, (o, _) in zip(views, spans))
    return list(zip(views[0::2], views[1::2])), buf, guard


@pytest.mark.parametrize("kind,hidden,in_dim", [("actor", (32,), 19), ("critic", (32,), 25), ("actor", (64, 96), 20),
                                                ("critic", (64, 96), 26)])
def test_every_element_once_and_nothing_beside_them(cuda, kind, hidden, in_dim):
    """Rows that start at any float, and sentinels behind every tensor: a store past the 6-row or
    1-row output layer, or past an in_dim-float row, lands on one; an element skipped or visited
    twice differs from the restatement (tau = 0.75: a second visit moves it again)."""
    rng = np.random.default_rng(200 + in_dim + len(hidden))
    online, target = _layers(rng, kind, hidden, in_dim), _layers(rng, kind, hidden, in_dim)
    net = _net(kind, _layers(rng, kind, hidden, in_dim), cuda)
    d_on, on_buf, on_guard = _carve(online, cuda)
    d_tg, tg_buf, tg_guard = _carve(target, cuda)
    on_before = on_buf.cpu().numpy().copy()
    net.polyak_(d_on, d_tg, 0.75)
    want = _assert_targets(_host(d_tg), _step(online, target, 0.75), (kind, hidden, in_dim))
    _assert_blob(net, want, (kind, hidden, in_dim))
    assert (_bits(tg_buf.cpu().numpy())[tg_guard] == SENTINEL).all()
    assert np.array_equal(_bits(on_buf.cpu().numpy()), _bits(on_before))
    for (W, b), (W0, b0) in zip(want, target):
        assert (_bits(W) != _bits(W0)).all() and (_bits(b) != _bits(b0)).all()        # every element moved


FOUR = [("actor", (32,), 19), ("critic", (64, 96), 26), ("actor", (64, 96), 20), ("critic", (32,), 25)]


@pytest.mark.parametrize("count", [2, 4])
def test_several_nets_in_one_launch(cuda, count):
    from ctr_reach_amd import _abi
    from ctr_reach_amd.policy import polyak_
    lib = _abi.load()
    rng = np.random.default_rng(300 + count)
    tau = 0.001
    shapes = FOUR[:count]
    online = [_layers(rng, *s) for s in shapes]
    target = [_layers(rng, *s) for s in shapes]
    together = [_net(s[0], _layers(rng, *s), cuda) for s in shapes]
    alone = [_net(s[0], _layers(rng, *s), cuda) for s in shapes]
    # a workgroup (256 threads, one per 16-B item) straddles the first two nets, and further ones
    items = [getattr(lib, "ctr_%s_blob_bytes" % n.NAME)(n._struct) // 16 for n in together]
    assert items[0] == 272 and items[0] % 256 != 0
    assert all(int(c) % 256 for c in np.cumsum(items)[:-1])
    d_on = [_device(o, cuda) for o in online]
    d_tg = [_device(t, cuda) for t in target]
    d_tg1 = [_device(t, cuda) for t in target]
    polyak_(list(zip(together, d_on, d_tg)), tau)
    for n, o, t in zip(alone, d_on, d_tg1):
        polyak_([(n, o, t)], tau)
    for m, s in enumerate(shapes):
        want = _assert_targets(_host(d_tg[m]), _step(online[m], target[m], tau), ("together", m, s))
        _assert_targets(_host(d_tg1[m]), want, ("alone", m, s))
        _assert_blob(together[m], want, ("together", m, s))
        _assert_blob(alone[m], want, ("alone", m, s))
        _assert_unchanged(d_on[m], online[m], ("online", m))


# (t, p) as bits: signed zeros; infinities against finite values and against each other (inf - inf);
# the largest finite float on opposite signs (p - t overflows); NaNs on either side; a pair whose
# difference is denormal (2^-126 and 1.5 * 2^-126: p - t = 2^-127); a pair whose difference is normal
# and whose product with either tau (0.001; 1 - 0.75) is denormal (2^-125 and 2^-124); denormal inputs
DENORMAL_DIFF = (0x00800000, 0x00C00000)
DENORMAL_PROD = (0x01000000, 0x01800000)
PAIRS = np.array([(0x00000000, 0x80000000), (0x80000000, 0x00000000), (0x80000000, 0x80000000),
                  (0x7F800000, 0x3F800000), (0x3F800000, 0xFF800000), (0x7F800000, 0x7F800000),
                  (0x7F800000, 0xFF800000), (0x7F7FFFFF, 0xFF7FFFFF), (0xFF7FFFFF, 0x7F7FFFFF),
                  (0x7FC00000, 0x3F800000), (0x3F800000, 0xFFC12345), DENORMAL_DIFF, DENORMAL_PROD,
                  (0x00000001, 0x807FFFFF)], dtype=np.uint32)


@pytest.mark.parametrize("tau", [0.001, 0.75])
def test_special_values(cuda, tau):
    rng = np.random.default_rng(400)
    kind, hidden, in_dim = "actor", (64, 96), 20
    online, target = _layers(rng, kind, hidden, in_dim), _layers(rng, kind, hidden, in_dim)
    for l in range(3):                                   # every pair in every matrix and in every bias
        for which in (0, 1):
            size = target[l][which].size
            where = rng.choice(size, min(PAIRS.shape[0], size), replace=False)
            _bits(target[l][which]).reshape(-1)[where] = PAIRS[:where.size, 0]
            _bits(online[l][which]).reshape(-1)[where] = PAIRS[:where.size, 1]
    # (the restatement keeps denormals: the two denormal pairs would come out differently flushed)
    t, p = (np.array([DENORMAL_DIFF[i], DENORMAL_PROD[i]], dtype=np.uint32).view(np.float32) for i in (0, 1))
    r = _reference(t, p, tau)
    flushed = _reference(t, p, tau)
    flushed[0] = t[0] if tau < 0.5 else p[0]
    assert _bits(r)[0] != _bits(flushed)[0] and _bits(r)[1] not in (_bits(t)[1], _bits(p)[1])
    net = _net(kind, _layers(rng, kind, hidden, in_dim), cuda)
    d_on, d_tg = _device(online, cuda), _device(target, cuda)
    net.polyak_(d_on, d_tg, tau)
    want = _step(online, target, tau)
    assert sum(int(np.isnan(W).sum() + np.isnan(b).sum()) for W, b in want) >= 15
    want = _assert_targets(_host(d_tg), want, ("specials", tau))
    _assert_blob(net, want, ("specials", tau))
    _assert_unchanged(d_on, online, "online")


def test_tau_one_is_load(cuda):
    """U(+-1/sqrt(fan_in)) online weights (no -0, finite differences): the targets become the online
    tensors, and the blob the one load_(online) packs."""
    rng = np.random.default_rng(500)
    kind, hidden, in_dim = "critic", (64, 96), 26
    online, target = _layers(rng, kind, hidden, in_dim), _layers(rng, kind, hidden, in_dim)
    net, twin = (_net(kind, _layers(rng, kind, hidden, in_dim), cuda) for _ in range(2))
    d_on, d_tg = _device(online, cuda), _device(target, cuda)
    net.polyak_(d_on, d_tg, 1.0)
    twin.load_(d_on)
    _assert_targets(_host(d_tg), _step(online, target, 1.0), "tau 1")
    _assert_targets(_host(d_tg), online, "tau 1: online")
    _assert_blob(net, online, "tau 1")
    assert np.array_equal(net.blob.cpu().numpy(), twin.blob.cpu().numpy())


def test_tau_zero_keeps_the_targets(cuda):
    rng = np.random.default_rng(600)
    kind, hidden, in_dim = "actor", (64, 96), 20
    online, target = _layers(rng, kind, hidden, in_dim), _layers(rng, kind, hidden, in_dim)
    net = _net(kind, _layers(rng, kind, hidden, in_dim), cuda)
    d_on, d_tg = _device(online, cuda), _device(target, cuda)
    net.polyak_(d_on, d_tg, 0.0)
    _assert_targets(_host(d_tg), _step(online, target, 0.0), "tau 0")
    _assert_targets(_host(d_tg), target, "tau 0: target")
    _assert_blob(net, target, "tau 0")


def test_a_captured_update_is_ordered_and_allocates_nothing(cuda):
    import torch
    from ctr_reach_amd.policy import polyak_
    rng = np.random.default_rng(700)
    tau = 0.75
    shapes = FOUR[:2]
    online = [_layers(rng, *s) for s in shapes]
    target = [_layers(rng, *s) for s in shapes]
    nets = [_net(s[0], _layers(rng, *s), cuda) for s in shapes]
    d_on = [_device(o, cuda) for o in online]
    d_tg = [_device(t, cuda) for t in target]
    triples = list(zip(nets, d_on, d_tg))
    polyak_(triples, tau)                                # (the kernel's first launch is not the captured one)
    torch.cuda.synchronize()
    target = [_step(o, t, tau) for o, t in zip(online, target)]
    before = torch.cuda.memory_allocated()
    polyak_(triples, tau)
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    target = [_step(o, t, tau) for o, t in zip(online, target)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # a synchronisation or an allocation in here raises
        polyak_(triples, tau)
    for _ in range(3):                                   # new online values, then the update, nothing waited for
        online = [_layers(rng, *s) for s in shapes]
        for dev, new in zip(d_on, online):
            for (W, b), (W1, b1) in zip(dev, new):
                W.copy_(torch.from_numpy(W1))
                b.copy_(torch.from_numpy(b1))
        graph.replay()
        target = [_step(o, t, tau) for o, t in zip(online, target)]
    torch.cuda.synchronize()
    for m in range(2):
        want = _assert_targets(_host(d_tg[m]), target[m], ("replayed", m))
        _assert_blob(nets[m], want, ("replayed", m))


def test_against_torch_lerp(cuda, capsys):
    """torch's own lerp_ may contract t + tau * d into one fused multiply-add, which rounds once where
    the restatement rounds the product first: |tau * d| * 2^-24 for that rounding, and one ulp of the
    result (2^-23 |t'|) for the two final roundings.  Derived, not measured; the measured maximum is
    printed."""
    import torch
    rng = np.random.default_rng(800)
    kind, hidden, in_dim, tau = "actor", (64, 96), 20, 0.001
    online, target = _layers(rng, kind, hidden, in_dim, scale=1.0), _layers(rng, kind, hidden, in_dim, scale=1.0)
    net = _net(kind, _layers(rng, kind, hidden, in_dim), cuda)
    d_on, d_tg = _device(online, cuda), _device(target, cuda)
    theirs = [tuple(t.clone().lerp_(p, tau).cpu().numpy() for t, p in zip(tp, op)) for tp, op in zip(d_tg, d_on)]
    net.polyak_(d_on, d_tg, tau)
    worst = 0.0
    for (W, b), (Wt, bt), ours, torchs in zip(online, target, _host(d_tg), theirs):
        for p, t, o, th in zip((W, b), (Wt, bt), ours, torchs):
            d = p.astype(np.float64) - t.astype(np.float64)
            o64, th64 = o.astype(np.float64), th.astype(np.float64)
            bound = 2.0 ** -24 * np.abs(tau * d) + 2.0 ** -23 * np.maximum(np.abs(o64), np.abs(th64))
            diff = np.abs(o64 - th64)
            assert (diff <= bound).all(), float((diff / bound).max())
            worst = max(worst, float((diff / np.spacing(np.abs(th)).astype(np.float64)).max()))
    with capsys.disabled():
        print("\npolyak_ against torch.lerp_ (tau = %g, U(-1, 1)): largest difference %.3g ulp" % (tau, worst))
