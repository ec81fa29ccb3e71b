"""eeg_gnn_ssl_amd — MI355X-native DCRNN forward/backward for the 19-electrode EEG graph.

Drop-in for the DCRNN hot path of tsy935/eeg-gnn-ssl (model/cell.py, model/model.py): the same
`nn.Module` classes, signatures and `state_dict` layout, computed by hand-written HIP kernels for
gfx950 behind a C ABI (include/eeg_dcrnn.h). 
"""
from . import ops, utils                                  # noqa: F401
from .device_data import (BalancedEpochSampler, DeviceDataset, EpochSampler, RecordingDataset, clip_table_classification, clip_table_detection,      # noqa: F401
                          clip_table_ssl, layout_recordings, clip_table_scan, clip_labels_detection, annotation_bins)
from .evaluation import DeviceEvaluator, DeviceSSLEvaluator     # noqa: F401
from .scan import Scanner, ScanResult, scores_from_scan_record     # noqa: F401
from .bootstrap import BootstrapResult, bootstrap_scores, paired_difference     # noqa: F401
from .interpret import OcclusionResult, occlusion_maps     # noqa: F401
from .statistics import ScalerFit, fit_scaler     # noqa: F401
from .resample import resample_recording, resample_recordings, resampled_length     # noqa: F401
from .edf import (EdfHeader, decode_edf, load_edf_recordings, read_edf_header, read_markers_classification,     # noqa: F401
                  read_markers_detection, read_markers_ssl, read_seizure_times, recording_ids, select_channels)
from .model.cell import DCGRUCell, DiffusionGraphConv     # noqa: F401
from .model.model import (DCGRUDecoder, DCRNNEncoder, DCRNNModel_classification,   # noqa: F401
                          DCRNNModel_nextTimePred)

__all__ = ["DCGRUCell", "DiffusionGraphConv", "DCRNNEncoder", "DCGRUDecoder",
           "DCRNNModel_classification", "DCRNNModel_nextTimePred", "DeviceDataset", "EpochSampler", "BalancedEpochSampler", "RecordingDataset", "clip_table_detection",
           "clip_table_ssl", "clip_table_classification", "layout_recordings", "DeviceEvaluator", "DeviceSSLEvaluator", "OcclusionResult",
           "occlusion_maps", "ScalerFit", "fit_scaler", "clip_table_scan", "clip_labels_detection", "annotation_bins", "Scanner", "ScanResult",
           "scores_from_scan_record", "BootstrapResult", "bootstrap_scores", "paired_difference", "resample_recording", "resample_recordings", "resampled_length", "EdfHeader", "read_edf_header",
           "select_channels", "read_seizure_times", "read_markers_detection", "read_markers_ssl", "read_markers_classification", "recording_ids",
           "decode_edf", "load_edf_recordings", "ops", "utils"]
