"""mla_hip: MI355X-native MLA alternating-unimodal training step (HIP kernels behind a C ABI).

Importing the package does not touch the GPU; the first op loads libmla_hip.so and raises
MLAHipError if it is missing (there is no CPU or eager fallback).
"""
from ._lib import MLAHipError, LIB_PATH  # noqa: F401
from .data import NpyBatcher, load_fbank, load_token  # noqa: F401
from .dist import Comm  # noqa: F401
from .encoder import ResNet18Encoder  # noqa: F401
from .feed import DeviceFeeder  # noqa: F401
from .frames import (FrameBatcher, decode_frames, frame_descriptors, make_lut, pick_frames, sample_augment,  # noqa: F401
                     sample_crop, sample_flip, sample_generator)
from .cav_feed import (CAVBatcher, decode_middle_frames, fbank_descriptors, image_descriptors, pick_middle_frame,  # noqa: F401
                       resize_center_crop, sample_fbank_aug)
from .m3ae_feed import M3AEBatcher, decode_images, jitter_descriptors, sample_jitter  # noqa: F401
from .modal3_feed import Modal3Batcher, mask_descriptors, random_mask  # noqa: F401
from .wav_feed import WavPart, clip_descriptors, extract_fbank, fbank_tables, read_wav, wav_part  # noqa: F401
from .resident_feed import ResidentFrameBatcher, ResidentStore, frame_table  # noqa: F401
from .model import AVClassifier, ConcatFusion, SharedHead  # noqa: F401
from .m3ae import CAVClassifier, ConcatFusion3, M3AEClassifier, M3AEEncoder, Modal3Classifier  # noqa: F401
from .clip import CLIPClassifier  # noqa: F401
from .clip_feed import CLIPFeatureBatcher, epoch_permutation, load_feature_tables  # noqa: F401
from .modulation import OGM  # noqa: F401
from .optim import FusedAdam, FusedSGD, cav_param_groups  # noqa: F401
from .plugin import GSPlugin  # noqa: F401
from .protocol import CrossEntropyLoss, DataParallel, setup_seed, weight_init  # noqa: F401
from .trainer import Evaluator, MLATrainer  # noqa: F401
from .joint import JointEvaluator, JointTrainer  # noqa: F401
from .qmf import QMFEvaluator, QMFHistory, QMFTrainer, attach_qmf_heads  # noqa: F401
from .metrics import ScoreStore  # noqa: F401
from .sweep import FusionSweep, SweepResult, fusion_grid  # noqa: F401
from .gate import GateSweep, GateSweepResult, gate_grid  # noqa: F401
from .fusion import FiLM, GatedFusion, SumFusion, attach_fusion  # noqa: F401
from . import torch_ops  # noqa: F401,E402  registers torch.ops.mla_hip.* (dispatch key CUDA; no other implementation)
