"""Wire-contract parity: our hand-built descriptors vs the FileDescriptorProtos
embedded in the reference's generated Go code (gogo api.pb.go and
metricssvc.pb.go). Field names, numbers, labels, types and the service
method signatures must be identical for kubelet / the exporter to interoperate.
The reference's side is recorded in tests/golden/reference/proto_contract.json:
what _fields / _services / the enum listing below give for its descriptors."""
import json
from pathlib import Path

from google.protobuf import descriptor_pb2

from rocm_k8s_device_plugin_amd.proto import deviceplugin as dp
from rocm_k8s_device_plugin_amd.proto import metricssvc as ms

CONTRACT = json.loads((Path(__file__).resolve().parent / "golden/reference/proto_contract.json").read_text())


def _ref_fields(ref):
    return {(m, f): (number, label, ftype, tn) for m, f, number, label, ftype, tn in ref["fields"]}


def _ref_services(ref):
    return {(s, m): (inp, out, sstream, cstream) for s, m, inp, out, sstream, cstream in ref["services"]}


def _fields(fdp):
    out = {}
    for m in fdp.message_type:
        for f in m.field:
            if f.type_name.endswith("Entry"):
                tn = "map"
            else:
                tn = f.type_name.split(".")[-1]
            out[(m.name, f.name)] = (f.number, f.label, f.type, tn)
    return out


def _services(fdp):
    return {(s.name, m.name): (m.input_type.split(".")[-1], m.output_type.split(".")[-1],
                               bool(m.server_streaming), bool(m.client_streaming))
            for s in fdp.service for m in s.method}


def _ours(desc):
    fdp = descriptor_pb2.FileDescriptorProto()
    desc.CopyToProto(fdp)
    return fdp


def test_deviceplugin_descriptor_matches_reference():
    ref = CONTRACT["deviceplugin"]
    ours = _ours(dp.FILE_DESCRIPTOR)
    assert ref["package"] == ours.package == "v1beta1"
    assert len(ref["fields"]) > 30 and len(ref["services"]) == 6
    assert _fields(ours) == _ref_fields(ref)
    assert _services(ours) == _ref_services(ref)


def test_metricssvc_descriptor_matches_reference():
    ref = CONTRACT["metricssvc"]
    ours = _ours(ms.FILE_DESCRIPTOR)
    assert ref["package"] == ours.package == "metricssvc"
    assert ref["fields"] and ref["services"]
    assert _fields(ours) == _ref_fields(ref)
    assert _services(ours) == _ref_services(ref)
    assert [e["name"] for e in ref["enums"]] == [e.name for e in ours.enum_type]
    assert [tuple(v) for v in ref["enums"][0]["values"]] == [(v.name, v.number) for v in ours.enum_type[0].value]


def test_roundtrip_wire_bytes():
    r = dp.ContainerAllocateResponse(envs={"A": "1"})
    r.devices.add(container_path="/dev/kfd", host_path="/dev/kfd", permissions="rw")
    b = r.SerializeToString()
    # field 1 (map entry, LEN) then field 3 (DeviceSpec, LEN)
    assert b[0] == (1 << 3 | 2) and (3 << 3 | 2) in b
    assert dp.ContainerAllocateResponse.FromString(b) == r
    d = dp.Device(ID="0000:05:00.0", health=dp.HEALTHY)
    d.topology.nodes.add(ID=1)
    assert dp.Device.FromString(d.SerializeToString()).topology.nodes[0].ID == 1


def test_constants():
    assert dp.VERSION == "v1beta1"
    assert dp.DEVICE_PLUGIN_PATH == "/var/lib/kubelet/device-plugins/"
    assert dp.KUBELET_SOCKET.endswith("device-plugins/kubelet.sock")
    assert (dp.HEALTHY, dp.UNHEALTHY) == ("Healthy", "Unhealthy")
