"""ubdvss_amd -- MI355X-native (gfx950) hot path of asmekal/ubdvss.

Host-side mirror of the reference's Python seams (NetConfig / NetManager / Model.predict,
ModelRunner.predict, SegmapManager.postprocess, losses.get_loss, Adam train step) over the
C ABI of ``libubd_hip.so`` (include/ubd.h).  PyTorch is used only for device memory, streams
and ``torch.distributed``.  There is no CPU fallback: importing the kernels without the built
library, or creating a model without an MI355X, raises.
"""
from .data_markup import ObjectMarkup, ClassifiedObjectMarkup  # noqa: F401
from .net import NetConfig, NetManager, PreprocessingType, Model, MultiscaleModel  # noqa: F401
from .model_runner import ModelRunner  # noqa: F401
from .segmap_manager import SegmapManager  # noqa: F401
from .object_patches import extract_objects_on_device  # noqa: F401
from .barcode_decoder import decode_patches_on_device, results_to_records, DecodedBarcode  # noqa: F401
from .barcode_decoder import decode_text_patches_on_device, text_results_to_records, DecodedText, CODE128  # noqa: F401
from .barcode_decoder import decode_width_patches_on_device, width_results_to_records, DecodedWidth, ITF, CODE39  # noqa: F401
from .barcode_decoder import UPCE, CODE93, CODABAR, upce_to_upca, full_ascii, code32_to_digits  # noqa: F401
from .barcode_decoder import decode_postal_patches_on_device, postal_results_to_records, DecodedPostal, kix_half_turned  # noqa: F401
from .barcode_decoder import POSTNET, PLANET, RM4SCC, KIX, POSTAL_SYMBOLOGIES  # noqa: F401
from .barcode_decoder import decode_matrix_patches_on_device, matrix_results_to_records, DecodedMatrix  # noqa: F401
from .barcode_decoder import DATAMATRIX, MATRIX_SYMBOLOGIES  # noqa: F401
from .augmentation import SegLinksImageAugmentation, AugmentationPlan, Stage, sample_plan, sample_photometric, apply_plan_to_markup  # noqa: F401
from . import losses  # noqa: F401
from .trainer import Trainer, Adam, History  # noqa: F401
from .data_generators import BatchGenerator, MetaInfo  # noqa: F401
from . import keras_callbacks  # noqa: F401
from .visualizations import Visualizer  # noqa: F401
from .evaluation import ImageResultCategories  # noqa: F401
from .result_saver import ResultSaver  # noqa: F401
