"""The three quantisers against the commit before their pass lifecycle was folded into one base (lvt_amd/modeling/vq): the same
C-ABI calls with the same scalar arguments, and the same bits in every output, gradient and piece of state.  `record()` drives a
quantiser alone through the public surface -- normalise_cl, straight_through_cl (joined, deferred + abandon_ema), indices_cl,
embed_cl, backward through st and bar -- at the smallest shapes that reach every geometry hook: 128 rows (P = 16) into two 16-d
codebooks (the generic-geometry search), one 128-d codebook (two 64-d groups: grouping, un-grouping, the shared index) and an
FSQ of projected width 6 (padded to 8).  A quarter of the codes start far away with running_size 0
(tests/test_gpu_codebook_restart_dp.py), so a restart-enabled pass restarts them.  The quantiser kernels sum in a fixed order
without atomics, so the digests are a property of the code and not of the run."""
import ctypes
import hashlib

import pytest
import torch

from util_models import vqvae_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 41
SHAPE = (8, 1, 4, 4)                                   # 128 rows, P = 16

QUANTISERS = {"dvq": 32, "single": 128, "fsq": 32}     # name -> channels D
#            EMA    restart cosine
VARIANTS = {"ema": (True, False, False), "ema_restart": (True, True, False), "ema_cosine": (True, False, True),
            "ema_cosine_restart": (True, True, True), "trained": (False, False, False)}
ENTRIES = [(q, v, m) for q in ("dvq", "single") for v in VARIANTS for m in ("f32", "f16x2")] + \
          [("fsq", "fsq", m) for m in ("f32", "f16x2")]

_HOST_ONLY = ("_bytes", "_uses_", "_fuses_", "_supported", "_is_gather", "lvt_last_error", "lvt_version", "lvt_device_info",
              "_partials")


def _plain(v):
    """A ctypes argument without its addresses: numbers as they are, structures (by value, by reference, in arrays) as the
    tuple of their fields that are no pointers."""
    v = getattr(v, "_obj", v)                          # byref(structure)
    if isinstance(v, ctypes.Structure):
        return tuple(_plain(getattr(v, name)) for name, typ in v._fields_ if typ is not ctypes.c_void_p)
    if isinstance(v, ctypes.Array):
        return tuple(_plain(e) for e in v)
    if isinstance(v, (int, float, bytes, type(None))):
        return v
    return type(v).__name__


class _Recorder:
    """Stands in for the ctypes handle: every enqueued entry point is logged with its scalar arguments, i.e. those that are not
    ctypes.c_void_p (the pattern of tests/test_gpu_fsq.py, which keeps the names alone)."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("lvt_") or any(s in name for s in _HOST_ONLY):
            return fn

        def logged(*a):
            self._calls.append((name, tuple(_plain(v) for v in a if not isinstance(v, ctypes.c_void_p))))
            return fn(*a)
        return logged


class _recording:
    """with _recording(mode) as calls: the math mode set and every C-ABI call of the block appended to `calls`."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from lvt_amd.hip import binding as L
        self.before, self.real, calls = L.get_math_mode(), L.lib, []
        L.set_math_mode(self.mode)
        handle = self.real()
        L.lib = lambda: _Recorder(handle, calls)
        return calls

    def __exit__(self, *exc):
        from lvt_amd.hip import binding as L
        torch.cuda.synchronize()
        L.lib = self.real
        L.set_math_mode(self.before)


def _summary(calls):
    """(names without the lvt_ prefix, sha256 of the whole record)."""
    return " ".join(n[4:] for n, _ in calls), hashlib.sha256(repr(calls).encode()).hexdigest()


def _sha(named):
    h = hashlib.sha256()
    for name, t in named:
        t = t.detach().cpu().contiguous()
        h.update(("%s %s %s|" % (name, t.dtype, tuple(t.shape))).encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def _build(kind, variant):
    """The quantiser on the device with its seeded state: every fourth code 1e3 away with running_size 0, the others with
    running_size 10 (tests/test_gpu_codebook_restart_dp.py); seeded projections for the FSQ."""
    from lvt_amd.modeling.vq import DVQEmbedding, FSQEmbedding, SingleVQEmbedding
    gen = torch.Generator().manual_seed(SEED + 1)
    if kind == "fsq":
        q = FSQEmbedding(2, [8, 5, 5], 32)
        sd = {k: (torch.randn(v.shape, generator=gen) / v.shape[-1] ** 0.5 if v.dim() == 2
                  else 0.2 * torch.randn(v.shape, generator=gen)) for k, v in q.state_dict().items()}
    else:
        ema, restart, cosine = VARIANTS[variant]
        q = DVQEmbedding(2, 64, 32, ema, cosine=cosine) if kind == "dvq" else SingleVQEmbedding(64, 128, ema, cosine=cosine)
        sd = {}
        for k, v in q.state_dict().items():
            if not k.endswith("embedding.weight"):
                continue
            w = torch.randn(v.shape, generator=gen)
            rs = torch.full((v.shape[0],), 10.0)
            w[0::4] += 1e3
            rs[0::4] = 0.0
            sd[k] = w
            if ema:
                prefix = k[:-len("embedding.weight")]
                sd[prefix + "running_size"] = rs
                sd[prefix + "running_sum"] = w * rs[:, None]
    q.load_state_dict(sd)
    q = q.to(DEV)
    if kind != "fsq" and VARIANTS[variant][1]:
        q.enable_restart(1.0, SEED)
    return q


def _state(q):
    named = sorted(q.state_dict().items())
    if q.restart_enabled:
        named += [(k, getattr(q, k)) for k in ("restart_pass", "restart_health", "restart_total")]
    return named


def record(kind, variant, mode):
    """-> {"calls": names, "args": sha256 of the (name, scalar arguments) record, stage: sha256 of what the stage left}."""
    gen = torch.Generator().manual_seed(SEED)
    D = QUANTISERS[kind]
    zs = [torch.randn(*SHAPE, D, generator=gen) for _ in range(5)]
    cots = [torch.randn(*SHAPE, D, generator=gen) for _ in range(4)]
    out = {}
    with _recording(mode) as calls:
        q = _build(kind, variant).train()
        for i in range(2):                                                     # two train passes, backward through st and bar
            z = zs[i].to(DEV).requires_grad_(True)
            st, bar = q.straight_through_cl(q.normalise_cl(z))
            pairs = [(t, g) for t, g in ((st, cots[2 * i]), (bar, cots[2 * i + 1])) if t.requires_grad]
            torch.autograd.backward([t for t, _ in pairs], [g.to(DEV) for _, g in pairs])
            grads = [("grad " + n, p.grad) for n, p in q.named_parameters() if p.grad is not None]
            out["train%d" % i] = _sha([("st", st), ("bar", bar), ("idx", q.last_indices), ("dz", z.grad)] + grads + _state(q))
            for p in q.parameters():
                p.grad = None
        st = q.straight_through_cl(q.normalise_cl(zs[2].to(DEV)), defer=True)    # a deferred pass that is given up
        q.abandon_ema()
        out["abandoned"] = _sha([("st", st), ("idx", q.last_indices)] + _state(q))
        q.eval()
        with torch.no_grad():
            st, bar = q.straight_through_cl(q.normalise_cl(zs[3].to(DEV)))
            out["eval"] = _sha([("st", st), ("bar", bar), ("idx", q.last_indices)] + _state(q))
            idx = q.indices_cl(q.normalise_cl(zs[4].to(DEV)))
            out["indices"] = _sha([("idx", idx)])
            out["embed"] = _sha([("emb", q.embed_cl(q.last_indices))] + _state(q))
    out["calls"], out["args"] = _summary(calls)
    return out


def record_fsq_step():
    """One PR-DVQVAE2 supervised step (forward + backward, 2 frames, f16x2) with FSQ levels [8, 8, 8] and EMA False
    -> (names, sha256 of the (name, scalar arguments) record)."""
    from lvt_amd.modeling import build_model
    from lvt_amd.utils.events import EventStorage
    cfg = vqvae_cfg(DEV)
    cfg.MODEL.CODEBOOK.FSQ.LEVELS = [8, 8, 8]
    cfg.MODEL.CODEBOOK.EMA = False
    torch.manual_seed(3)
    model = build_model(cfg)
    model.train()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    with _recording("f16x2") as calls:
        with EventStorage(0):
            losses = model([{"image": x[i].numpy()} for i in range(2)], mode="supervised")
        assert set(losses) == {"loss_reconstruction"}
        sum(losses.values()).backward()
    return _summary(calls)


STAGES = ("train0", "train1", "abandoned", "eval", "indices", "embed")


@pytest.mark.parametrize("entry", ENTRIES, ids="-".join)
def test_quantiser_matches_the_parent_commit(entry):
    kind, variant, mode = entry
    got = record(*entry)
    print(got)
    args, names = PARENT_CALLS["-".join(entry)]
    assert got["calls"].split() == names.split()
    assert got["args"] == args
    # (the codebook quantisers search exactly in either arithmetic: one set of digests for both modes)
    want = PARENT_DIGESTS["-".join(entry) if kind == "fsq" else "%s-%s" % (kind, variant)]
    assert {s: got[s] for s in STAGES} == dict(zip(STAGES, want))


def test_fsq_supervised_step_issues_the_calls_of_the_parent_commit():
    names, args = record_fsq_step()
    print(names, args)
    assert names.split() == PARENT_FSQ_STEP[0].split()
    assert args == PARENT_FSQ_STEP[1]


# Recorded from the parent commit with record() / record_fsq_step() (that commit's package, this file unchanged):
PARENT_DIGESTS = {        # in the order of STAGES
    "dvq-ema": ("e7998b53170e20370aebc7813c1e42f58b11ab2c8f9eef1aa06f4efd12cb5211",
                "a58c9fbad5ad527b556d463611d10f75499407a3d2b7559a6c925cae74d96eb4",
                "6769a8497a29de03f497aa3e8076beaf5468d4a0ffde312f06451e5063bb5f06",
                "8ea5f93b24e3f5631f4e2b08adcc4001ce5fcb5b13427d5567e44bec8cace05f",
                "eff1ce242108cd956e074884b0fbea800eef9cf7e08dd17b2834343149317bf1",
                "a775dca028f193d574fb69da9c17f8740c0db41862a619b6cc01b028644eadfe"),
    "dvq-ema_restart": ("3570e0fe03312d4ea47bf03728ed790d665e511da9e3c5da86bd02e1303dd6db",
                        "e3591eccb34596417b0e11e4d366cf8fde5f83956cde1fd3b929e03b29d2d43a",
                        "cd704e2b95a373b1e2cd82bbbe1e7d4dd646c36fc05343e8d58d681ac8f17006",
                        "7f532dd5e4a13405422fadd1e8117a49689831721c7c6c45534c946c06b40067",
                        "43dbb3dae909f0686f66e8a838ed3eeaac71f88c40221a68d5d64d17d00f5bf8",
                        "1c950c3db210e9db533bf155846b80089af9e753cf048a1da6fa7ebc40768450"),
    "dvq-ema_cosine": ("f47a93d7c2019a4dbec835673c7bdccb90adb157914f506154bb08a7e15d961a",
                       "c07ecae47e9e1762f10dd9a25833701b1cda0711ebc3c6053eb48b7b14500753",
                       "bf08c1625d66061cc72fb198a4a8e07e72afe10e84162224aed3cb5149994034",
                       "8a3bfadd7e3e0ef00573a0c63013a3c56e730c8ca5d79e4ed11f3b0b1a3f446d",
                       "edded5bd1c0aa1df660f333e48adaf08095285f095947ce68543f340c2db1b08",
                       "d9370a8cba359018ba9e8bd211f904006f39661ddc0d9d4a9b3c82ff2c4dad89"),
    "dvq-ema_cosine_restart": ("66ea0f73eaaf96fdf672757486e93b71e11800350bff6d92053adda54f4a1731",
                               "03e39bf3d28015a0a73904d6e0b0835ef1f2d67574ea9e5a22e89f7245b00382",
                               "812d0015061b5647f0a2891489da6ec472577724902d1f3a5900625b318bdca7",
                               "6e022ae3a8d336168e2a63b23a8c558f3b45c546ba1f699fa6e6afe7e45584b3",
                               "b21df35e782d2eaa6a787b4f626316460526fee903daba7f608dd5cd4988a13a",
                               "c5a3ccc7478e6308e935a288df306024d6c820706637a932d86ac5ce30f377df"),
    "dvq-trained": ("91f3ad62d5f1e4fd2b0082b81f1d505cd62aef709b71d432927531648494075a",
                    "c7f2869fb415407f43487a6ef35de057962c3d57153c7898ec3119d13260b32f",
                    "7ac46f4296cd8973c9369ff58c5f35cc18b5e325c9f2535cfb7206f1cf79d69b",
                    "28ebf2885434726ed9711d4cb3ccaddf19b1526e882d9cb14a1a346098af6a0c",
                    "c94f287cb65d5be53ddaa31dc90f6c2be5799dcb64472c21bd064b6c50e03385",
                    "2af76db190af4fa7c4add8cf1c629aa4dbf87506f9e36da71df8fbafaf92fcc2"),
    "single-ema": ("02691e2d5dd0e42b4f9720944269d1b542608b1c43f6c311a8425852322f39c3",
                   "7a4e6d49d6eddac3e37a2833bef90d01b2cf1f3e280f71cdd61f2009240e3b43",
                   "5f503ff0c3ebeb772d70f1420a81671bf26c8330ec6c39ed56b07a2616470ffd",
                   "526e432807092920fac0090cbab67462d70b40e1fdb32a2ad82f6b0b43491bca",
                   "be4e26b82bdde8823be9ccc4b2517a96e337a301f6ceebd53bcd1efe76e94552",
                   "67c430694209a4923f09841ce08fc96b9e0f855947ec2a192fc44a622d2d124d"),
    "single-ema_restart": ("ea7a7f61dce2cb8d94a00fac37ab2201e345fa305d2919ea54d2d6f6517ec834",
                           "b172f33ac1c8d3a947ba98e2ef7a79c4cdcdf40a865506628ab5e3d13a8e968c",
                           "77cddbf7cd16650ceb528e3bb33b1ec476e116b6dbc9cf580daca99a69e513eb",
                           "c2fb91df05ba0f976c1311f338a6a47bd326dae305d7f6ac96817db79f8dbed0",
                           "fd6e914a3c373048cec653bbdee9bac4705bc5a67eb2ab871b9c1c2d7896dcf1",
                           "4aea22e66f7854e2e8ede8359fcd3e685dfdf3864a7a176c7c5f8883d8681d85"),
    "single-ema_cosine": ("4d2dc588cdf9087135fdc2dc484de0f6860a5add3d1a505702b66d569fb4c8fa",
                          "f9f6596fbe9668a6b381f8d9b861daf9d668dd021bb581d391b14f49a1ac07e5",
                          "1a8f63efc3082c97ad74a8b3312b273ec6d957a60dee707e8114a1c90f04d5d1",
                          "eae25d215fa99f7f426dc3415f86b26c32762f240df2f22b8179458ea8cdc63d",
                          "57a10315d607666e2453776843a87e68641abfb7ced5f6c49ba8ae4328d27825",
                          "07eb21f4420bfb76c697fae70af7f58622fcc62b1a2491d19f0ade25b76d2a0e"),
    "single-ema_cosine_restart": ("499976261d56b2a5db606c4ec936194407e53c135d6ba4112371377a1bcfed34",
                                  "13ff371dcfd701647bd92f5fa540bfc35745b5415250334a6c9b6343fca2e379",
                                  "15d02f5dd685b7631d806722889009c051d34ce00f74f42ff12610296981f9da",
                                  "aa28839e048625abf9923e9d57261bbed66a543d3f42dd0e1e506e3c81767991",
                                  "f733df66cc129b0a1697d2785a4b7a6358b694e869593f7003bfe3dbad027ac5",
                                  "c94571cb73aea78c9a27155af68023e0cfc50f7a332546f2738bdde4c30fb05c"),
    "single-trained": ("76d7951be354543be35cb74487232a99b41e94697d34bb80106b0c1e97c47625",
                       "23f92e314c36096870329e6021f497ab71e06bcc620e37ca965dcde9b01fddbc",
                       "0b2194e2875d4b5574de0c68bf175ba3cdfef901037826c1a0936a644a7d2ebc",
                       "eaa2c537045e38c009986186937d1993eeee827da68d1deae996d8008fe54800",
                       "7f0df8427ce959997a012dece88655f962e69ce2237a72e783283cc5e8634f4e",
                       "68703f2f0264ad86878889da3a32d45573670dab04c8b1872586e94b126db199"),
    "fsq-fsq-f32": ("40b6dcb96a3e7ae081753712b2185a76e08ba4146abe3730056a34c86232a65f",
                    "b068570ad80adad557bafe41d275fbce59d6dfbc95d172ab5afb0baed9f71481",
                    "96371921e748d0aaafb1e97ababd5507af5ba2cc8366fbe1d325c04e939c5c28",
                    "d4f5f8ee9eb97fd8fa5a7a7c68eaf0b658c786a1a5cddd2e9306d7b6fc137864",
                    "a7e7af9a7e719903ce2574f2a69281d48ff406c2edcffbbac36bb45b4273e600",
                    "e046d574b7951275cbf8fe83cc3c21d40f778d90f7626897e00c30a294735fc2"),
    "fsq-fsq-f16x2": ("f99695b6860f36fcf0a9e674b0a654fe96c4244cca8c8a3d332070b166db1ee8",
                      "a53dfff469e26e8ccdc5a95f1baea0e2eeaf4b5d219975fc5474c06e48c8f359",
                      "f992c85eb598d1b980b75575bdab04207ff7dd3c5726abd344c67f96a4a31cc1",
                      "f4a68338cc6f93f089fe74b92412fa6bbc830067eba88f0054ada89feabc2fd8",
                      "a7e7af9a7e719903ce2574f2a69281d48ff406c2edcffbbac36bb45b4273e600",
                      "5402946d30cf11d6c7a9ac843a9955764c33ea8070036ee87212dca79552e352"),
}
PARENT_CALLS = {          # entry -> (sha256 of the (name, scalar arguments) record, the names)
    "dvq-ema-f32": (
        "a81ef9555f886a6dc28b76ae91bc36fd0fe0e15a48b6668729950d8f784ccc92",
        "vq_nearest vq_gather vq_ema_accumulate vq_ema_finalize vq_gather vq_nearest vq_gather vq_ema_accumulate "
        "vq_ema_finalize vq_gather vq_nearest vq_gather vq_ema_accumulate vq_nearest vq_gather vq_ema_accumulate "
        "vq_ema_finalize vq_gather vq_nearest vq_gather"),
    "dvq-ema-f16x2": (
        "23fd1766ba29aedd73b020c65616f19e732f8d88a9e3c8e85ad32cbcdec843e6",
        "vq_nearest vq_gather amax vq_ema_accumulate vq_ema_finalize vq_gather amax vq_nearest vq_gather vq_ema_accumulate "
        "vq_ema_finalize vq_gather amax vq_nearest vq_gather vq_ema_accumulate vq_nearest vq_gather vq_ema_accumulate "
        "vq_ema_finalize vq_gather amax vq_nearest vq_gather"),
    "dvq-ema_restart-f32": (
        "af762e551fa53000991d14512badd8529bd8ec3cf8ebe0fc35ada203b95d88cd",
        "vq_nearest vq_gather vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart vq_gather vq_nearest vq_gather "
        "vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart vq_gather vq_nearest vq_gather vq_ema_accumulate "
        "vq_restart_candidates vq_nearest vq_gather vq_ema_accumulate vq_ema_finalize vq_gather vq_nearest vq_gather"),
    "dvq-ema_restart-f16x2": (
        "90682a632395cdf5450798d85b44762e587bf2fcf0a51aed7a9ae21fb05a8249",
        "vq_nearest vq_gather amax vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart vq_gather amax vq_nearest "
        "vq_gather vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart vq_gather amax vq_nearest vq_gather "
        "vq_ema_accumulate vq_restart_candidates vq_nearest vq_gather vq_ema_accumulate vq_ema_finalize vq_gather amax "
        "vq_nearest vq_gather"),
    "dvq-ema_cosine-f32": (
        "00e2dce0d6a5fe3a95510756cc32759421be6a847c9bd50d5b49d2c04fea42e4",
        "l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd vq_gather l2norm_groups_bwd "
        "l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd vq_gather l2norm_groups_bwd "
        "l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate "
        "vq_ema_finalize l2norm_groups_fwd vq_gather l2norm_groups_fwd vq_nearest vq_gather"),
    "dvq-ema_cosine-f16x2": (
        "4e92e1b1f3f7003219dae6b849aecc97bfc36a5bf45dbf40b8feef795f74dfad",
        "l2norm_groups_fwd vq_nearest vq_gather amax vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd vq_gather "
        "l2norm_groups_bwd l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd vq_gather "
        "l2norm_groups_bwd l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate l2norm_groups_fwd vq_nearest vq_gather "
        "vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd vq_gather l2norm_groups_fwd vq_nearest vq_gather"),
    "dvq-ema_cosine_restart-f32": (
        "f9f26688d7494fbd9f9b44555c8da652af8090da4ae61017b386263b580b6b99",
        "l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart "
        "l2norm_groups_fwd vq_gather l2norm_groups_bwd l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate "
        "vq_restart_candidates vq_ema_finalize_restart l2norm_groups_fwd vq_gather l2norm_groups_bwd l2norm_groups_fwd "
        "vq_nearest vq_gather vq_ema_accumulate vq_restart_candidates l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate "
        "vq_ema_finalize l2norm_groups_fwd vq_gather l2norm_groups_fwd vq_nearest vq_gather"),
    "dvq-ema_cosine_restart-f16x2": (
        "da24951725c0b4d13f30999465a7a99bb24fb556fd49d94d8a8db55f4d0135a2",
        "l2norm_groups_fwd vq_nearest vq_gather amax vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart "
        "l2norm_groups_fwd vq_gather l2norm_groups_bwd l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate "
        "vq_restart_candidates vq_ema_finalize_restart l2norm_groups_fwd vq_gather l2norm_groups_bwd l2norm_groups_fwd "
        "vq_nearest vq_gather vq_ema_accumulate vq_restart_candidates l2norm_groups_fwd vq_nearest vq_gather vq_ema_accumulate "
        "vq_ema_finalize l2norm_groups_fwd vq_gather l2norm_groups_fwd vq_nearest vq_gather"),
    "dvq-trained-f32": (
        "b4d0a61e024ac0f889c89c2f2886b44be462ff396fde5d8a006eb2c3f5240ae8",
        "vq_nearest vq_gather vq_gather vq_ema_accumulate vq_nearest vq_gather vq_gather vq_ema_accumulate vq_nearest vq_gather "
        "vq_nearest vq_gather vq_gather vq_nearest vq_gather"),
    "dvq-trained-f16x2": (
        "443a09dea3272b68bee81c80b6d56e2bad0e218bab51dc0c8414ba564a6d6d57",
        "vq_nearest vq_gather amax vq_gather vq_ema_accumulate vq_nearest vq_gather vq_gather vq_ema_accumulate vq_nearest "
        "vq_gather vq_nearest vq_gather vq_gather vq_nearest vq_gather"),
    "single-ema-f32": (
        "58a4e5921e2bcb9ca8fa7a79ab8e1ae6d4ee46f73e8cf6d22dc762aaf40c7790",
        "gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate vq_ema_finalize vq_gather gemm_f32 vq_argmax_scores vq_gather "
        "vq_ema_accumulate vq_ema_finalize vq_gather gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate gemm_f32 "
        "vq_argmax_scores vq_gather vq_ema_accumulate vq_ema_finalize vq_gather gemm_f32 vq_argmax_scores vq_gather"),
    "single-ema-f16x2": (
        "f6203febb647413912e3ae22da2aff38f1533e479efc7972ad4ed85aaa403e57",
        "amax amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate vq_ema_finalize vq_gather amax amax amax gemm_f32 "
        "vq_argmax_scores vq_gather amax vq_ema_accumulate vq_ema_finalize vq_gather amax amax amax gemm_f32 vq_argmax_scores "
        "vq_gather amax vq_ema_accumulate amax amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate vq_ema_finalize "
        "vq_gather amax amax amax gemm_f32 vq_argmax_scores vq_gather amax"),
    "single-ema_restart-f32": (
        "299de715325dfe8e7005340106d66400517d72e287ced34ed85d2ed8f8d3a4d5",
        "gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart vq_gather gemm_f32 "
        "vq_argmax_scores vq_gather vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart vq_gather gemm_f32 "
        "vq_argmax_scores vq_gather vq_ema_accumulate vq_restart_candidates gemm_f32 vq_argmax_scores vq_gather "
        "vq_ema_accumulate vq_ema_finalize vq_gather gemm_f32 vq_argmax_scores vq_gather"),
    "single-ema_restart-f16x2": (
        "1d59beffae4a4e29c7964b30b23f522dba32d155d1fbb96d3885af8d262cd69d",
        "amax amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart "
        "vq_gather amax amax amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate vq_restart_candidates "
        "vq_ema_finalize_restart vq_gather amax amax amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate "
        "vq_restart_candidates amax amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate vq_ema_finalize vq_gather "
        "amax amax amax gemm_f32 vq_argmax_scores vq_gather amax"),
    "single-ema_cosine-f32": (
        "0c52a364596ec16357894adfb786a337d8c94c9e1090d63a39b1c9f408e297ba",
        "l2norm_groups_fwd gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd vq_gather "
        "l2norm_groups_bwd l2norm_groups_fwd gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate vq_ema_finalize "
        "l2norm_groups_fwd vq_gather l2norm_groups_bwd l2norm_groups_fwd gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate "
        "l2norm_groups_fwd gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd vq_gather "
        "l2norm_groups_fwd gemm_f32 vq_argmax_scores vq_gather"),
    "single-ema_cosine-f16x2": (
        "8bf03c0ab6b8cea5221babbc93aa44a1f89e87c0cf8d0140c0b399ae216c3ad6",
        "l2norm_groups_fwd amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd "
        "vq_gather amax l2norm_groups_bwd l2norm_groups_fwd amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate "
        "vq_ema_finalize l2norm_groups_fwd vq_gather amax l2norm_groups_bwd l2norm_groups_fwd amax gemm_f32 vq_argmax_scores "
        "vq_gather amax vq_ema_accumulate l2norm_groups_fwd amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate "
        "vq_ema_finalize l2norm_groups_fwd vq_gather amax l2norm_groups_fwd amax gemm_f32 vq_argmax_scores vq_gather amax"),
    "single-ema_cosine_restart-f32": (
        "ae4890d66bac36d2b3b44ed1258c8076875f08492f2327f03134251f5e5faec1",
        "l2norm_groups_fwd gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart "
        "l2norm_groups_fwd vq_gather l2norm_groups_bwd l2norm_groups_fwd gemm_f32 vq_argmax_scores vq_gather vq_ema_accumulate "
        "vq_restart_candidates vq_ema_finalize_restart l2norm_groups_fwd vq_gather l2norm_groups_bwd l2norm_groups_fwd gemm_f32 "
        "vq_argmax_scores vq_gather vq_ema_accumulate vq_restart_candidates l2norm_groups_fwd gemm_f32 vq_argmax_scores "
        "vq_gather vq_ema_accumulate vq_ema_finalize l2norm_groups_fwd vq_gather l2norm_groups_fwd gemm_f32 vq_argmax_scores "
        "vq_gather"),
    "single-ema_cosine_restart-f16x2": (
        "aab89da7cb82262b8300ef9f45ed1b44aa229af7c6928c54fa254cd60cfc2b0e",
        "l2norm_groups_fwd amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate vq_restart_candidates "
        "vq_ema_finalize_restart l2norm_groups_fwd vq_gather amax l2norm_groups_bwd l2norm_groups_fwd amax gemm_f32 "
        "vq_argmax_scores vq_gather amax vq_ema_accumulate vq_restart_candidates vq_ema_finalize_restart l2norm_groups_fwd "
        "vq_gather amax l2norm_groups_bwd l2norm_groups_fwd amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate "
        "vq_restart_candidates l2norm_groups_fwd amax gemm_f32 vq_argmax_scores vq_gather amax vq_ema_accumulate "
        "vq_ema_finalize l2norm_groups_fwd vq_gather amax l2norm_groups_fwd amax gemm_f32 vq_argmax_scores vq_gather amax"),
    "single-trained-f32": (
        "7a11056bb31442967994b684000083b5a583063e20214f65a2fe5f439cb7a04f",
        "gemm_f32 vq_argmax_scores vq_gather vq_gather vq_ema_accumulate gemm_f32 vq_argmax_scores vq_gather vq_gather "
        "vq_ema_accumulate gemm_f32 vq_argmax_scores vq_gather gemm_f32 vq_argmax_scores vq_gather vq_gather gemm_f32 "
        "vq_argmax_scores vq_gather"),
    "single-trained-f16x2": (
        "ee3c7425d941581a139691a659566469fe66c56216cab3cad86308117eb9a7e0",
        "amax amax gemm_f32 vq_argmax_scores vq_gather amax vq_gather amax vq_ema_accumulate amax amax gemm_f32 "
        "vq_argmax_scores vq_gather amax vq_gather amax vq_ema_accumulate amax amax gemm_f32 vq_argmax_scores vq_gather amax "
        "amax amax gemm_f32 vq_argmax_scores vq_gather amax vq_gather amax amax amax gemm_f32 vq_argmax_scores vq_gather amax"),
    "fsq-fsq-f32": (
        "467895048c55218298205879fbb78899fc53e667fe3c7eabeb7b63df10a2ce54",
        "gemm_f32 fsq_fwd gemm_f32 gemm_f32 gemm_f32 colsum fsq_bwd gemm_f32 colsum gemm_f32 gemm_f32 fsq_fwd gemm_f32 gemm_f32 "
        "gemm_f32 colsum fsq_bwd gemm_f32 colsum gemm_f32 gemm_f32 fsq_fwd gemm_f32 gemm_f32 fsq_fwd gemm_f32 gemm_f32 fsq_fwd "
        "fsq_decode gemm_f32"),
    "fsq-fsq-f16x2": (
        "94b8c2b8aee3b4b05ef69625185de38532301d6820407755c4bf0d239e6044d1",
        "amax amax gemm_f32 fsq_fwd amax gemm_f32 amax gemm_f32 gemm_f32 colsum fsq_bwd gemm_f32 colsum gemm_f32 amax amax "
        "gemm_f32 fsq_fwd amax gemm_f32 amax gemm_f32 gemm_f32 colsum fsq_bwd gemm_f32 colsum gemm_f32 amax amax gemm_f32 "
        "fsq_fwd amax gemm_f32 amax amax gemm_f32 fsq_fwd amax gemm_f32 amax amax gemm_f32 fsq_fwd fsq_decode amax gemm_f32"),
}
PARENT_FSQ_STEP = (
    "amax_multi to_channels_last conv3d_pack_weights_multi conv3d_weight_images conv3d_fwd conv3d_fwd_parity conv3d_fwd "
    "conv3d_fwd conv3d_fwd conv3d_fwd conv3d_fwd gemm_f32 fsq_fwd gemm_f32 conv3d_pack_weights_multi conv3d_weight_images "
    "conv3d_fwd conv3d_fwd conv3d_fwd conv3d_fwd conv3d_fwd conv3d_bwd_data_phases convt4_fwd_act mse_fwd mse_bwd tanh_bwd "
    "conv3d_bwd_weight colsum conv3d_fwd conv3d_bwd_weight conv3d_fwd_parity conv3d_bwd_weight conv3d_bwd_data "
    "conv3d_bwd_weight conv3d_fwd conv3d_bwd_weight conv3d_bwd_data conv3d_bwd_weight conv3d_fwd conv3d_bwd_weight conv3d_fwd "
    "gemm_f32 gemm_f32 colsum fsq_bwd gemm_f32 colsum gemm_f32 conv3d_bwd_weight conv3d_bwd_data conv3d_bwd_weight conv3d_fwd "
    "conv3d_bwd_weight conv3d_bwd_data conv3d_bwd_weight conv3d_fwd conv3d_bwd_weight conv3d_fwd conv3d_bwd_weight "
    "conv3d_bwd_data_phases conv3d_bwd_weight",
    "07ae93b2044ff20749fcd8e539ec58532624975b681e64825af4bbc0308ad32c")
