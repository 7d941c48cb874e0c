"""Drop-in for the reference's mad_icp.src.pybind.pypeline — re-exports mad_icp_amd.pybind.pypeline (MI355X implementation)."""
from mad_icp_amd.pybind.pypeline import *  # noqa: F401,F403
from mad_icp_amd.records import (T_F32, T_F64, T_NONE, T_U32, TIME_FIELD_NAMES, RecordLayout,  # noqa: F401  (Pipeline.
                                 Source, attribute_of, layout_of)                                # computeRecordsStamped's and
                                                                                                 # computeSourcesStamped's helpers)
