"""Host restatements of the four stand-alone policy kernels (k_gauss_mlp_policy, k_lstm_policy, k_gleet_policy, k_qnet_argmax) and of
the Philox draw they share (sample_action, mbx_rlepso.hpp), with the checks tests/test_policy_exact.py applies to them.

Three kinds of statement are made about a kernel, from the strongest down:

  * BIT FOR BIT.  v_mfma_f32_16x16x4_f32 with the accumulator started at the bias is one float32 fma chain per output unit, k ascending.
    `fma32` is a correctly rounded float32 fma on numpy arrays: the product of two float32 is exact in float64 (48 bits), the sum with c is
    split by a two-sum into a rounded part and its error, the rounded part is moved to the neighbour with an odd last bit when the error is
    not zero (round to odd), and the float64 -> float32 cast then rounds once (a 53-bit round-to-odd value has more than two guard bits over
    24, subnormal results included).  float32(float64(a) * b + c) rounds twice and is wrong on about one triple in 2^29 near a tie (`fma32_double`, a planted
    defect).  `chain32` is the chain; the Q-network, the LSTM's gate pre-activations and its mu head are held to it exactly.
  * THE DRAW.  `normal64` is sample_action's deviate in float64: Philox words (x, y) of counter (j, MBX_SITE_POLICY, gen + 1, episode)
    under the instance's seed, u1 = ((x >> 8) + 1) 2^-24, u2 = (y >> 8) 2^-24, n = sqrt(-2 ln u1) cos(2 pi u2).  The device evaluates the same expression
    in float32 on v_log_f32 / v_cos_f32.  `E32` is the scale of float32 Box-Muller: the largest |numpy float32 evaluation - normal64| over a
    set of words; the device is allowed 16 E32 on the deviate, i.e. 16 E32 sigma + 4 float32 ulp on the action (`check_draws`).  A clamp /
    re-fold decision closer than that to its edge may fall on either side and is counted.
  * THE E_ref RULE (this project's, tests/test_les.py) for whatever passes through tanh / exp / sigmoid: per quantity E_ref is the largest
    |torch CPU float32 evaluation - float64 restatement| over the inputs of the test, and the kernel must lie within 4 E_ref + 4 float32 ulp
    of the float64 restatement, element-wise (`rule_fraction`).  Inputs are the float32-rounded states widened to float64, weights the
    packed float32 buffers of include/mbx.h widened to float64.

Every restatement takes an optional `defect`: the planted mistakes the checks must reject (tests/test_policy_exact.py shows each rejected).
"""
import functools
import math

import numpy as np

from oracle import oracle

F32 = np.float32
SITE_POLICY = 15                         # MBX_SITE_POLICY (include/mbx_layout.h)
SC_GEN, SC_EPISODE = 6, 7                # MBX_SC_GEN / MBX_SC_EPISODE
POLICY_RLEPSO, POLICY_RLPSO = 0, 1       # MBX_POLICY_* (include/mbx.h)
DRAW_FACTOR = 16                         # the device's allowance on the deviate, in E32

DRAW_DEFECTS = ('sine', 'words_zw', 'index_plus_1', 'gen_not_plus_1', 'episode_zero', 'seed_high_dropped')
CHAIN_DEFECTS = ('k_descending', 'pairwise', 'bias_last', 'double_rounding')
RULE_DEFECTS = ('gleet_biased_variance', 'gleet_scale_dropped', 'rlpso_sigma_affine')


def ulp32(x):
    """float32 spacing at |x| (x float64), as float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def f32_64(x):
    """Round to float32, widen to float64: what a kernel's (float) cast makes of a float64 state."""
    return np.asarray(x, dtype=np.float64).astype(F32).astype(np.float64)


# ================================================================================================ exact float32 fma and the chain
def fma32(a, b, c):
    """Correctly rounded float32 a * b + c on numpy arrays (finite inputs)."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    p = a * b                                              # exact: 24 x 24 bits, exponent range far inside float64's
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                        # two-sum: p + c = s + err exactly
    s, err = np.broadcast_arrays(s, err)
    s = s.copy()
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even                                # round to odd: of the two float64 around p + c, the one with an odd last bit
    s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    return s.astype(F32)


def fma32_double(a, b, c):
    """The double-rounding form (a planted defect): float64 sum rounded to nearest, then to float32."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    return (a * b + c).astype(F32)


def chain32(x, Wt, bias, defect=None):
    """[B, K] x Wt [K, N] + bias [N] -> [B, N] float32: per unit ONE fma chain, k ascending, started at the bias."""
    x, Wt, bias = np.asarray(x, dtype=F32), np.asarray(Wt, dtype=F32), np.asarray(bias, dtype=F32)
    B, K = x.shape
    N = Wt.shape[1]
    assert Wt.shape[0] == K and bias.shape == (N,)
    fma = fma32_double if defect == 'double_rounding' else fma32
    if defect == 'pairwise':
        terms = [fma(x[:, k, None], Wt[k][None, :], np.zeros((B, N), F32)) for k in range(K)] + [np.broadcast_to(bias, (B, N)).copy()]
        while len(terms) > 1:
            terms = [(terms[i] + terms[i + 1]).astype(F32) if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        return terms[0]
    acc = np.zeros((B, N), F32) if defect == 'bias_last' else np.broadcast_to(bias, (B, N)).copy()
    for k in (range(K - 1, -1, -1) if defect == 'k_descending' else range(K)):
        acc = fma(x[:, k, None], Wt[k][None, :], acc)
    return (acc + bias[None, :]).astype(F32) if defect == 'bias_last' else acc


def relu32(x):
    return np.where(x > 0, x, F32(0)).astype(F32)


# ================================================================================================ the draw
def philox_words(seeds, n_index, gen_words, episodes, defect=None):
    """Philox words of sample_action for every (instance, component): uint32 [B, n_index, 4].  gen_words is the counter word, i.e. the
    scalar block's generation + 1."""
    seeds = [int(s) for s in (seeds if np.ndim(seeds) else [seeds])]          # (never through a float array: the high words matter)
    out = np.empty((len(seeds), n_index, 4), dtype=np.uint64)
    for b, seed in enumerate(seeds):
        g, e = int(np.atleast_1d(gen_words)[b]), int(np.atleast_1d(episodes)[b])
        if defect == 'gen_not_plus_1':
            g -= 1
        if defect == 'episode_zero':
            e = 0
        if defect == 'seed_high_dropped':
            seed &= 0xFFFFFFFF
        for j in range(n_index):
            out[b, j] = oracle.philox(seed, j + 1 if defect == 'index_plus_1' else j, SITE_POLICY, g, e)
    return out


def uniforms64(words, defect=None):
    x, y = (words[..., 2], words[..., 3]) if defect == 'words_zw' else (words[..., 0], words[..., 1])
    return ((x >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24, (y >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def normal64_of_words(words, defect=None):
    u1, u2 = uniforms64(words, defect)
    ang = 2.0 * math.pi * u2
    return np.sqrt(-2.0 * np.log(u1)) * (np.sin(ang) if defect == 'sine' else np.cos(ang))


def normal64(seed, j, gen_word, episode):
    """The deviate of sample_action(rng{seed, gen_word, episode}, j, ...) in float64."""
    w = np.array(oracle.philox(int(seed), int(j), SITE_POLICY, int(gen_word), int(episode)), dtype=np.uint64)
    return float(normal64_of_words(w))


def normal32_of_words(words):
    """The same expression evaluated in numpy float32, operation by operation as sample_action writes it: log2, the constant -2 ln 2, sqrt,
    cos(2 pi u2) (the device's v_cos_f32 takes u2 in revolutions; numpy has to form the float32 product 2 pi u2)."""
    x, y = words[..., 0], words[..., 1]
    u1 = ((x >> np.uint64(8)) + np.uint64(1)).astype(F32) * F32(5.9604644775390625e-8)
    u2 = (y >> np.uint64(8)).astype(F32) * F32(5.9604644775390625e-8)
    r = np.sqrt(F32(-1.3862943611198906) * np.log2(u1))
    return (r * np.cos(F32(2.0 * math.pi) * u2)).astype(F32)


def e32_of_words(words):
    return float(np.abs(normal32_of_words(words).astype(np.float64) - normal64_of_words(words)).max())


E32_WORDS = 200_000


@functools.lru_cache(maxsize=None)
def e32():
    """E32 over the file's fixed word set: 2e5 Philox words of sample_action's own counters (1000 seeds, half with the high word set,
    200 components, generation words 1 .. 4, episodes 0 / 1) -- the draw-defect test uses a prefix of the same set."""
    return e32_of_words(draw_word_set(E32_WORDS))


@functools.lru_cache(maxsize=None)
def draw_word_set(n):
    per = 200
    nb = n // per
    seeds = [(0x9E3779B97F4A7C15 + 977 * k) & 0xFFFFFFFFFFFFFFFF if k % 2 else 3 + 11 * k for k in range(nb)]
    return philox_words(seeds, per, [1 + k % 4 for k in range(nb)], [(k // 4) % 2 for k in range(nb)]).reshape(-1, 4)


def draw_word_set_meta(n):
    """(seeds, gen words, episodes) of draw_word_set(n), per block of 200 components."""
    nb = n // 200
    seeds = [(0x9E3779B97F4A7C15 + 977 * k) & 0xFFFFFFFFFFFFFFFF if k % 2 else 3 + 11 * k for k in range(nb)]
    return seeds, [1 + k % 4 for k in range(nb)], [(k // 4) % 2 for k in range(nb)]


def post64(variant, mu, sigma, n):
    """The agent's post-processing of a = mu + sigma n in float64: clamp to [0, 1] (RLEPSO, LDE, GLEET), or RL-PSO's re-fold
    |a - 0.5| >= 0.5 -> (a + 3 sigma - mu) * (1/6 sigma) (the reference's rl_pso_agent.py:33-34, precedence as written there)."""
    mu, sigma, n = (np.asarray(v, dtype=np.float64) for v in (mu, sigma, n))
    a = mu + sigma * n
    if variant == POLICY_RLPSO:
        return np.where(np.abs(a - 0.5) >= 0.5, (a + 3.0 * sigma - mu) * (1.0 / 6.0 * sigma), a)
    return np.clip(a, 0.0, 1.0)


def sample32(variant, mu, sigma, words):
    """sample_action in numpy float32 (no contraction, like the translation unit): what a correct device computes up to its transcendentals."""
    mu, sigma = np.asarray(mu, dtype=F32), np.asarray(sigma, dtype=F32)
    a = (mu + (sigma * normal32_of_words(words)).astype(F32)).astype(F32)
    if variant == POLICY_RLPSO:
        fold = (((a + (F32(3) * sigma).astype(F32)).astype(F32) - mu).astype(F32) * ((F32(1) / F32(6)) * sigma).astype(F32)).astype(F32)
        return np.where(np.abs((a - F32(0.5)).astype(F32)) >= F32(0.5), fold, a).astype(F32)
    return np.clip(a, F32(0), F32(1))


def check_draws(got, mu, sigma, n64, variant, E32, max_undecided=0.001):
    """|a - post64(mu, sigma, n64)| <= 16 E32 sigma + 4 float32 ulp for every element; where the float64 pre-image lies further than that
    from 0 and 1 the clamp / re-fold decision must be the host's (a clamped value exactly 0 or 1); closer elements may take either side and
    are counted.  Returns (None, stats) or (a message, stats)."""
    got, mu, sigma, n64 = (np.asarray(v, dtype=np.float64) for v in (got, mu, sigma, n64))
    a = mu + sigma * n64
    tol = DRAW_FACTOR * E32 * sigma + 4 * ulp32(a)
    near = (np.abs(a) <= tol) | (np.abs(a - 1.0) <= tol)
    want = post64(variant, mu, sigma, n64)
    err = np.abs(got - want)
    if variant == POLICY_RLPSO:
        other = np.where(np.abs(a - 0.5) >= 0.5, a, (a + 3.0 * sigma - mu) * (1.0 / 6.0 * sigma))      # the other side of the decision
        err = np.where(near, np.minimum(err, np.abs(got - other)), err)
        folded = np.abs(a - 0.5) >= 0.5
    else:
        folded = (a < 0) | (a > 1)
        exact_edge = ~near & folded
        if np.any(got[exact_edge] != want[exact_edge]):
            return 'a clamped value is not exactly 0 or 1', {}
    stats = {'n': int(got.size), 'undecided': int(near.sum()), 'worst': float((err / tol).max()), 'folded': int((folded & ~near).sum())}
    if not np.all(np.isfinite(got)):
        return 'non-finite action', stats
    bad = err > tol
    if bad.any():
        return f'{int(bad.sum())} of {got.size} draws outside 16 E32 sigma + 4 ulp (worst {stats["worst"]:.3g} of the bound)', stats
    if near.sum() > max_undecided * got.size and near.sum() > 0:
        return f'{int(near.sum())} of {got.size} elements sit on a clamp edge', stats
    return None, stats


def draw_reject_share(got, mu, sigma, n64, variant, E32):
    """Share of the elements that check_draws rejects (element-wise part only)."""
    got, mu, sigma, n64 = (np.asarray(v, dtype=np.float64) for v in (got, mu, sigma, n64))
    a = mu + sigma * n64
    tol = DRAW_FACTOR * E32 * sigma + 4 * ulp32(a)
    return float((np.abs(got - post64(variant, mu, sigma, n64)) > tol).mean())


# ================================================================================================ the E_ref rule
def e_ref(ref32, want64):
    return float(np.abs(np.asarray(ref32, dtype=np.float64) - np.asarray(want64, dtype=np.float64)).max())


def rule_tol(want64, E):
    return 4 * E + 4 * ulp32(want64)


def rule_fraction(got, want64, E):
    """Largest |got - want| / (4 E + 4 float32 ulp): the kernel passes at <= 1."""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    assert got.shape == want64.shape and np.all(np.isfinite(got)), 'shape / non-finite'
    return float((np.abs(got - want64) / rule_tol(want64, E)).max())


# ================================================================================================ Gaussian MLP (mbx_gauss_mlp)
def gauss_net_floats(IN, H1, H2, A):
    return IN * H1 + H1 + H1 * H2 + H2 + H2 * A + A


def gauss_split(w, IN, H1, H2, A):
    """Packed buffer -> [(W1t, b1, W2t, b2, W3t, b3) of the mu net, the same of the sigma net] (include/mbx.h, mbx_gauss_mlp)."""
    w = np.asarray(w, dtype=F32)
    n = gauss_net_floats(IN, H1, H2, A)
    assert w.size == 2 * n
    nets = []
    for base in (0, n):
        o, parts = base, []
        for rows, cols in ((IN, H1), (H1, H2), (H2, A)):
            parts.append(w[o:o + rows * cols].reshape(rows, cols)); o += rows * cols
            parts.append(w[o:o + cols]); o += cols
        nets.append(parts)
    return nets


def seeded_gauss(rs, IN, H1, H2, A, mu_bias=None, scale=1.0):
    """Seeded packed weights, torch.nn.Linear's U(-1/sqrt(fan_in), 1/sqrt(fan_in)) times `scale`; mu_bias overwrites the mu net's last bias."""
    parts = []
    for net in range(2):
        for rows, cols in ((IN, H1), (H1, H2), (H2, A)):
            k = scale / math.sqrt(rows)
            parts += [rs.uniform(-k, k, rows * cols), rs.uniform(-k, k, cols)]
        if net == 0 and mu_bias is not None:
            parts[-1] = np.full(A, mu_bias)
    return np.concatenate(parts).astype(F32)


def _mlp(parts, x, xp):
    W1, b1, W2, b2, W3, b3 = parts
    h = xp.maximum(x @ W1 + b1, 0)
    h = xp.maximum(h @ W2 + b2, 0)
    return h @ W3 + b3


def gauss64(w, dims, min_sigma, max_sigma, variant, x, defect=None):
    """(mu, sigma) [B, A] in float64 from the packed float32 weights and the float32-rounded states."""
    nets = [[p.astype(np.float64) for p in parts] for parts in gauss_split(w, *dims)]
    x = f32_64(x)
    lo, hi = float(F32(min_sigma)), float(F32(max_sigma))              # the struct carries them as float
    mu = (np.tanh(_mlp(nets[0], x, np)) + 1.0) / 2.0
    t = (np.tanh(_mlp(nets[1], x, np)) + 1.0) / 2.0
    if variant == POLICY_RLPSO and defect != 'rlpso_sigma_affine':
        return mu, np.clip(t, lo, hi)
    return mu, t * (hi - lo) + lo


def gauss_torch32(w, dims, min_sigma, max_sigma, variant, x):
    """The same network as torch CPU float32 modules evaluate it (the E_ref side of the rule)."""
    import torch
    nets = [[torch.from_numpy(np.ascontiguousarray(p)) for p in parts] for parts in gauss_split(w, *dims)]
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64).astype(F32))

    def mlp(parts):
        W1, b1, W2, b2, W3, b3 = parts
        return torch.addmm(b3, torch.relu(torch.addmm(b2, torch.relu(torch.addmm(b1, xt, W1)), W2)), W3)
    mu = (torch.tanh(mlp(nets[0])) + 1.) / 2.
    t = (torch.tanh(mlp(nets[1])) + 1.) / 2.
    sigma = torch.clamp(t, min=min_sigma, max=max_sigma) if variant == POLICY_RLPSO else t * (max_sigma - min_sigma) + min_sigma
    return mu.numpy(), sigma.numpy()


# ================================================================================================ LSTM policy (mbx_lstm_policy)
def lstm_floats(IN, H, A):
    return (IN + H) * 4 * H + 4 * H + 2 * H * A + 2 * A


def lstm_split(w, IN, H, A):
    """Packed buffer -> dict: Wg [IN + H, 4H] (W_ih^T stacked on W_hh^T: the kernel's k runs over [x | h]), bg, WmuT, WsgT [H, A], bmu, bsg."""
    w = np.asarray(w, dtype=F32)
    assert w.size == lstm_floats(IN, H, A)
    o, out = 0, {}
    for name, shape in (('Wg', (IN + H, 4 * H)), ('bg', (4 * H,)), ('WmuT', (H, A)), ('WsgT', (H, A)), ('bmu', (A,)), ('bsg', (A,))):
        n = int(np.prod(shape))
        out[name] = w[o:o + n].reshape(shape); o += n
    return out


def seeded_lstm(rs, IN, H, A, scale=1.0):
    k = scale / math.sqrt(H)
    return rs.uniform(-k, k, lstm_floats(IN, H, A)).astype(F32)


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def lstm_gates32(parts, x, h, defect=None):
    """Exact float32 gate pre-activations [B, 4H] (torch.nn.LSTM's row order i, f, g, o)."""
    xs = np.concatenate([np.asarray(x, dtype=np.float64).astype(F32), np.asarray(h, dtype=F32)], axis=1)
    return chain32(xs, parts['Wg'], parts['bg'], defect)


def lstm_cell64(gates, c):
    """(h', c') in float64 from the float32 gate chains and c."""
    g = np.asarray(gates, dtype=np.float64)
    H = g.shape[1] // 4
    gi, gf, gg, go = sigmoid64(g[:, :H]), sigmoid64(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), sigmoid64(g[:, 3 * H:])
    cn = gf * np.asarray(c, dtype=np.float64) + gi * gg
    return go * np.tanh(cn), cn


def lstm_cell_torch32(gates, c):
    """The same cell update in torch CPU float32 on the same gate pre-activations (the E_ref side)."""
    import torch
    g, ct = torch.from_numpy(np.ascontiguousarray(gates, dtype=F32)), torch.from_numpy(np.ascontiguousarray(c, dtype=F32))
    H = g.shape[1] // 4
    gi, gf, gg, go = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
    cn = gf * ct + gi * gg
    return (go * torch.tanh(cn)).numpy(), cn.numpy()


def sigmoid_torch32(x):
    import torch
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x, dtype=F32))).numpy()


# ================================================================================================ Q-network (mbx_qnet)
def qnet_split(w, IN=99, W=100, depth=4, A=4):
    w = np.asarray(w, dtype=F32)
    dims = [IN] + [W] * depth + [A]
    o, layers = 0, []
    for a, b in zip(dims[:-1], dims[1:]):
        layers.append((w[o:o + a * b].reshape(a, b), w[o + a * b:o + a * b + b])); o += a * b + b
    assert o == w.size
    return layers


def qnet32(w, x, defect=None):
    """Q values [B, 4] float32: five chain32 layers with exact ReLU; action = first maximum."""
    a = np.asarray(x, dtype=np.float64).astype(F32)
    layers = qnet_split(w)
    for li, (Wt, b) in enumerate(layers):
        a = chain32(a, Wt, b, defect)
        if li < len(layers) - 1:
            a = relu32(a)
    return a, a.argmax(1).astype(np.int32)


def seeded_qnet(rs, tie=True, IN=99, W=100, depth=4, A=4):
    """Seeded Q-network; with `tie` the last layer's columns 1 and 3 are identical (non-negative weights, bias 0.5) and columns 0 and 2 are
    non-positive with bias -0.5: behind a ReLU Q1 == Q3 > 0 > Q0, Q2 for every input, so the first maximum is action 1."""
    dims = [IN] + [W] * depth + [A]
    parts = []
    for li, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        k = 1.0 / math.sqrt(a)
        Wt, bias = rs.uniform(-k, k, (a, b)), rs.uniform(-k, k, b)
        if tie and li == len(dims) - 2:
            Wt = np.abs(Wt)
            Wt[:, 3] = Wt[:, 1]
            Wt[:, 0] *= -1
            Wt[:, 2] *= -1
            bias = np.array([-0.5, 0.5, -0.5, 0.5])
        parts += [Wt.reshape(-1), bias]
    return np.concatenate(parts).astype(F32)


# ================================================================================================ GLEET actor
def gleet_forward(actor, x, defect=None):
    """metabox_amd.agent.gleet_agent.Actor.features + distribution restated on the module's own parameters, in the parameters' dtype
    (float64 after actor.double()), with the planted defects.  x [B, ps, 27] -> (mu, sigma) [B, ps]."""
    import torch

    def norm(t):
        mean = t.mean((1, 2)).view(-1, 1, 1)
        return (t - mean) / torch.sqrt(t.var((1, 2), unbiased=defect != 'gleet_biased_variance').view(-1, 1, 1) + 1e-05)

    def layer(L, h, q=None):
        m = L.MHA_sublayer.MHA
        q = h if q is None else q
        Q = torch.einsum('bne,hek->hbnk', q, m.W_query)
        K = torch.einsum('bne,hek->hbnk', h, m.W_key)
        V = torch.einsum('bne,hek->hbnk', h, m.W_val)
        scale = 1.0 if defect == 'gleet_scale_dropped' else 1 / math.sqrt(m.dk)
        heads = torch.matmul(torch.softmax(scale * torch.matmul(Q, K.transpose(2, 3)), dim=-1), V)
        h = norm(torch.einsum('hbnk,hke->bne', heads, m.W_out) + h)
        return norm(L.FFandNorm_sublayer.FF(h) + h)
    with torch.no_grad():
        n = actor.node_dim
        h = layer(actor.encoder[0], actor.embedder(x[:, :, :n]))
        q = actor.embedder_for_decoder(torch.cat((actor.embedder(x[:, :, n:2 * n]), actor.embedder(x[:, :, 2 * n:])), dim=-1))
        z = layer(actor.decoder[0], h, q)
        mu = (torch.tanh(actor.mu_net(z)) + 1.) / 2.
        sigma = (torch.tanh(actor.sigma_net(z)) + 1.) / 2. * (actor.max_sigma - actor.min_sigma) + actor.min_sigma
    return mu[..., 0].numpy(), sigma[..., 0].numpy()


def gleet_scores_head0(actor64, x):
    """Scaled scores of every particle's query against every key in the encoder layer's head 0, float64: [ps, ps] (row = query)."""
    import torch
    with torch.no_grad():
        m = actor64.encoder[0].MHA_sublayer.MHA
        h = actor64.embedder(x[None, :, :actor64.node_dim])[0]
        return ((h @ m.W_query[0]) @ (h @ m.W_key[0]).T / math.sqrt(m.dk)).numpy()


def gleet_inputs(rs, NP, actor64, recorded=None):
    """The planted swarms, float32-valued float64 arrays [n, NP, 27]: uniform features; features times 8 sorted so that particle 0's
    head-0 encoder scores ascend with the key index from key 1 on (the running maximum of the online softmax moves in every chunk of four);
    one outlier particle; memories equal to the features (the reset state); the recorded swarms where the population matches."""
    import torch
    out = {}
    out['uniform'] = rs.rand(NP, 27)
    for _ in range(50):
        big = rs.rand(NP, 27) * 8.0
        S = gleet_scores_head0(actor64, torch.from_numpy(f32_64(big)))
        # the query particle goes first: one whose own key scores among the lowest of its row, so that from key 1 on the scores ascend and
        # the first chunk's maximum is already below the second chunk's
        p = int(np.argmin((S < np.diag(S)[:, None]).sum(1)))
        rest = np.array([j for j in np.argsort(S[p], kind='stable') if j != p], dtype=np.int64)
        order = np.concatenate([[p], rest])
        if chunk_max_moves(S[p][order]):
            break
    else:
        raise AssertionError('no swarm with ascending scores found')
    out['sorted_x8'] = big[order]
    outl = rs.rand(NP, 27)
    outl[NP // 2] = 40.0 * (1 + rs.rand(27))
    out['outlier'] = outl
    mem = rs.rand(NP, 27)
    mem[:, 9:18] = mem[:, :9]; mem[:, 18:] = mem[:, :9]
    out['reset_state'] = mem
    if recorded is not None and recorded.shape[1] == NP:
        for k in range(recorded.shape[0]):
            out[f'recorded{k}'] = recorded[k]
    return {k: f32_64(v) for k, v in out.items()}


def chunk_max_moves(scores):
    """True when the running maximum of the online softmax (keys four at a time) changes in every chunk."""
    m, ok = -np.inf, True
    for j0 in range(0, len(scores), 4):
        mn = max(m, scores[j0:j0 + 4].max())
        ok, m = ok and mn > m, mn
    return ok
