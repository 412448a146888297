from .evaluator import (BitsEvaluator, CodesExtractor, DatasetEvaluator, DatasetEvaluators, FrameQualityEvaluator, MSEEvaluator,
                        PredictionQualityEvaluator, VTSampler, build_evaluator, inference_on_dataset)
from .quality import frame_quality_reference, prediction_quality_reference, ssim_loss_reference

__all__ = ["BitsEvaluator", "CodesExtractor", "DatasetEvaluator", "DatasetEvaluators", "FrameQualityEvaluator", "MSEEvaluator",
           "PredictionQualityEvaluator", "VTSampler", "build_evaluator", "frame_quality_reference", "inference_on_dataset",
           "prediction_quality_reference", "ssim_loss_reference"]
