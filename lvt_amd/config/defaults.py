"""Default config tree.  Key names and default values are the reference's config surface
(vidgen/config/defaults.py:3-170); they are part of the drop-in boundary because the shipped YAML
files (configs/vqvae/*.yaml, configs/vt/*.yaml) and CLI overrides are merged against this tree.
Written as a flat table (one row per leaf) rather than attribute assignments."""
from .config import CfgNode

_TABLE = [
    ('MODEL.DEVICE', 'cuda'),
    ('MODEL.META_ARCHITECTURE', 'ACAIModel'),
    ('MODEL.PIXEL_MEAN', [0.0]),
    ('MODEL.PIXEL_STD', [1.0]),
    ('MODEL.IGNORE_INDEX', -100),
    ('MODEL.INIT_TYPE', 'normal'),
    ('MODEL.INIT_VARIANCE', 0.02),
    ('MODEL.AUTOREGRESSIVE.NAME', ''),
    ('MODEL.AUTOREGRESSIVE.VT.NC', 0),
    ('MODEL.AUTOREGRESSIVE.VT.NV', 0),
    ('MODEL.AUTOREGRESSIVE.VT.KERNEL', ()),
    ('MODEL.AUTOREGRESSIVE.VT.STRIDE', ()),
    ('MODEL.AUTOREGRESSIVE.VT.D', 0),
    ('MODEL.AUTOREGRESSIVE.VT.DA', 0),
    ('MODEL.AUTOREGRESSIVE.VT.DE', 0),
    ('MODEL.AUTOREGRESSIVE.VT.BLOCKS_E', ()),
    ('MODEL.AUTOREGRESSIVE.VT.N_HEAD_E', ()),
    ('MODEL.AUTOREGRESSIVE.VT.BLOCKS_D', ()),
    ('MODEL.AUTOREGRESSIVE.VT.N_HEAD_D', ()),
    ('MODEL.AUTOREGRESSIVE.VT.N_PRIME', 0),
    ('MODEL.AUTOREGRESSIVE.VT.PAD_VALUE', -1),
    ('MODEL.AUTOREGRESSIVE.VT.SHARE_P', True),
    ('MODEL.AUTOREGRESSIVE.VT.SHARE_EMBEDDINGS', False),
    ('MODEL.AUTOREGRESSIVE.VT.CLASS_NUM', 0),
    ('MODEL.AUTOREGRESSIVE.VT.DROPOUT', 0.0),        # residual dropout of every attention layer's two branches; 0.0: off
    ('MODEL.ENCODER.WEIGHTS', ''),
    ('MODEL.ENCODER.NAME', ''),
    ('MODEL.ENCODER.IN_CHANNELS', 1),
    ('MODEL.ENCODER.NF', 16),
    ('MODEL.ENCODER.RES_CHANNELS', 0),
    ('MODEL.ENCODER.OUT_CHANNELS', 16),
    ('MODEL.ENCODER.NORM', ''),
    ('MODEL.ENCODER.N_LAYERS', 0),
    ('MODEL.ENCODER.SPECTRAL', False),
    ('MODEL.ENCODER.OUT_ACTIVATION', ''),
    ('MODEL.GENERATOR.WEIGHTS', ''),
    ('MODEL.GENERATOR.NAME', ''),
    ('MODEL.GENERATOR.IN_CHANNELS', 16),
    ('MODEL.GENERATOR.NF', 16),
    ('MODEL.GENERATOR.RES_CHANNELS', 0),
    ('MODEL.GENERATOR.OUT_CHANNELS', 3),
    ('MODEL.GENERATOR.NORM', ''),
    ('MODEL.GENERATOR.N_LAYERS', 0),
    ('MODEL.GENERATOR.SPECTRAL', False),
    ('MODEL.GENERATOR.OUT_ACTIVATION', ''),
    ('MODEL.CODEBOOK.NUM', 1),
    ('MODEL.CODEBOOK.SIZE', 512),
    ('MODEL.CODEBOOK.DIM', 256),
    ('MODEL.CODEBOOK.WEIGHTS', ''),
    ('MODEL.CODEBOOK.EMA', False),
    ('MODEL.CODEBOOK.BETA', 1.0),
    ('MODEL.CODEBOOK.RESTART.ENABLED', False),       # re-seed dead EMA codes from encoder rows + codebook health
    ('MODEL.CODEBOOK.RESTART.THRESHOLD', 1.0),       # dead: running_size below it and no row won in the pass; 0.0: monitoring only
    ('MODEL.CODEBOOK.COSINE', False),                # l2-normalised (cosine) lookup on unit-row EMA codebooks
    ('MODEL.CODEBOOK.FSQ.LEVELS', []),               # finite scalar quantisation, e.g. [8, 8, 8]: SIZE = prod(LEVELS)
    ('INPUT.FORMAT', 'L'),
    ('INPUT.N_FRAMES_PER_VIDEO_TRAIN', -1),
    ('INPUT.N_FRAMES_PER_VIDEO_TEST', -1),
    ('INPUT.SCALE_TO_ZEROONE', True),
    ('INPUT.PREPARE_SLICES_TRAIN', False),
    ('GAN_MODE_ON', False),
    ('DATASETS.TRAIN', ()),
    ('DATASETS.TEST', ()),
    ('DATALOADER.NUM_WORKERS', 4),
    ('DATALOADER.SAMPLER_TRAIN', 'TrainingSampler'),
    ('SOLVER.MAX_ITER', 40000),
    ('SOLVER.SUPERVISED_MAX_ITER', -1),
    ('SOLVER.LR_SCHEDULER_NAME', 'Identity'),
    ('SOLVER.GAMMA', 0.1),
    ('SOLVER.STEPS', ()),
    ('SOLVER.WARMUP_ITERS', -1),
    ('SOLVER.WARMUP_FACTOR', 0.01),
    ('SOLVER.WARMUP_METHOD', 'linear'),
    ('SOLVER.OPTIMIZER_NAME', 'adam'),
    ('SOLVER.LR_G', 0.0001),
    ('SOLVER.LR_D', 0.0004),
    ('SOLVER.WEIGHT_DECAY.BASE_G', 0.0),
    ('SOLVER.WEIGHT_DECAY.BIAS_G', 0.0),
    ('SOLVER.WEIGHT_DECAY.NORM_G', 0.0),
    ('SOLVER.WEIGHT_DECAY.BASE_D', 0.0),
    ('SOLVER.WEIGHT_DECAY.BIAS_D', 0.0),
    ('SOLVER.WEIGHT_DECAY.NORM_D', 0.0),
    ('SOLVER.ADAM.BETA1_G', 0.9),
    ('SOLVER.ADAM.BETA2_G', 0.9),
    ('SOLVER.ADAM.BETA1_D', 0.9),
    ('SOLVER.ADAM.BETA2_D', 0.999),
    ('SOLVER.RMSPROP.ALPHA_G', 0.99),
    ('SOLVER.RMSPROP.ALPHA_D', 0.99),
    ('SOLVER.RMSPROP.MOMENTUM_G', 0.0),
    ('SOLVER.RMSPROP.MOMENTUM_D', 0.0),
    ('SOLVER.ACCUMULATION_STEPS', 1),
    ('SOLVER.CHECKPOINT_PERIOD', 50000),
    ('SOLVER.IMS_PER_BATCH', 32),
    ('SOLVER.D_UPDATE_RATIO', 1),
    ('SOLVER.D_INIT_ITERS', -1),
    ('SOLVER.MAXUP', False),
    ('SOLVER.CLIP_GRADIENTS.ENABLED', False),        # detectron2's keys (the reference dropped them): solver/clip.py
    ('SOLVER.CLIP_GRADIENTS.CLIP_TYPE', 'norm'),     # "norm": global 2-norm over all optimizers; "value": elementwise clamp
    ('SOLVER.CLIP_GRADIENTS.CLIP_VALUE', 1.0),
    ('SOLVER.CLIP_GRADIENTS.NORM_TYPE', 2.0),
    ('SOLVER.MODEL_EMA.ENABLED', False),             # Polyak-averaged weights kept by the fused optimizer steps: solver/ema.py
    ('SOLVER.MODEL_EMA.DECAY', 0.9999),
    ('SOLVER.MODEL_EMA.WARMUP', True),               # decay of update t: min(DECAY, (1 + t) / (10 + t))
    ('LOSS.PIXEL.ONN', False),
    ('LOSS.PIXEL.LAMBDA', 1.0),
    ('LOSS.PIXEL.MODE', 'l2'),
    ('LOSS.SSIM.LAMBDA', 0.0),                       # weight of the 1 - SSIM term of the reconstruction loss; 0.0: off
    ('LOSS.GAN.ONN', False),
    ('LOSS.GAN.LAMBDA_G', 1.0),
    ('LOSS.GAN.LAMBDA_D', 1.0),
    ('LOSS.GAN.REAL_LABEL', 1.0),
    ('LOSS.GAN.FAKE_LABEL', 0.0),
    ('LOSS.GAN.MODE', 'wgan'),
    ('TEST.EXPECTED_RESULTS', []),
    ('TEST.EVAL_PERIOD', 0),
    ('TEST.N_SAMPLES', 0),
    ('TEST.EVALUATORS', ''),
    ('TEST.VT_SAMPLER.VQ_VAE.CFG', ''),
    ('TEST.VT_SAMPLER.VQ_VAE.ENCODER_WEIGHTS', ''),
    ('TEST.VT_SAMPLER.VQ_VAE.GENERATOR_WEIGHTS', ''),
    ('TEST.VT_SAMPLER.VQ_VAE.CODEBOOK_WEIGHTS', ''),
    ('TEST.VT_SAMPLER.N_PRIME', 5),
    ('TEST.VT_SAMPLER.NUM_SAMPLES', 10),
    # truncated sampling (modeling/autoregressive/sampling.py): temperature of every draw, top-k (0: off), top-p (1.0: off)
    ('TEST.VT_SAMPLER.TEMPERATURE', 1.0),
    ('TEST.VT_SAMPLER.TOP_K', 0),
    ('TEST.VT_SAMPLER.TOP_P', 1.0),
    ('OUTPUT_DIR', './output'),
    ('SEED', -1),
    ('CUDNN_BENCHMARK', True),
    ('VIS_PERIOD', 100000000000),
    ('VERSION', 1),
    ('GLOBAL.HACK', 1.0),
]


def _build():
    root = CfgNode()
    for key, value in _TABLE:
        node = root
        parts = key.split(".")
        for p in parts[:-1]:
            if p not in node:
                dict.__setitem__(node, p, CfgNode())
            node = node[p]
        dict.__setitem__(node, parts[-1], value)
    return root


_C = _build()
