from .frame import optimize_params_frame
from .sequence import SequenceBatch, optimize_params_sequence, optimize_params_sequences, optimize_shape_sequence

__all__ = ["optimize_params_frame", "optimize_params_sequence", "optimize_params_sequences", "SequenceBatch",
           "optimize_shape_sequence"]
