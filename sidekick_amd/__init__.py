"""sidekick_amd — MI355X-native quACK power-sum engine (gfx950 HIP kernels
behind the C ABI in include/quack_hip.h).  See DESIGN.md."""
from .quack import (  # noqa: F401
    CoefficientVector, Context, DeviceFlowQuacks, DeviceFlowSnapshots, DeviceSenderLog, FlowQuacks, FlowSnapshots, ModularInteger, PowerSumQuackU32, PowerSumQuackU64,
    SenderLogStep, SenderStep, SenderSteps, Snapshots, arithmetic, decode_segments, device_count, drain_segments, emit_wire, flows_diff, flows_lookup, flows_merge,
    get_context, ingest_wire, ingest_wire_queue, roots, sender_step, sender_steps, snapshot_flows, snapshot_segments, to_coeffs_segments, update_segments, wire_max,
)
from ._lib import P32, P64, QuackError, UndecodableError  # noqa: F401

__version__ = "0.1.0"
