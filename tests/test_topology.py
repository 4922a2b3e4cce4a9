"""Topology extractor against the documented known answers (no GPU)."""
import json
import os

import numpy as np

from common import GOLDEN, load_topo
import pytest

from flobaroid_amd.topology import Topology, parse_urdf

# the reference's robot descriptions (model/<name>.urdf), stored as data fixtures
URDF_DIR = os.path.join(GOLDEN, "urdf")

_URDF = """<robot name="t">
  <link name="world_box"/>
  <joint name="fix0" type="fixed"><origin xyz="1 2 3" rpy="0 0 0.5"/><origin xyz="9 9 9"/><parent link="world_box"/><child link="a"/></joint>
  <link name="a"><inertial><mass value="2"/><origin xyz="0.1 0 0" rpy="0 0 1.5707963267948966"/>
     <inertia ixx="1" ixy="0" ixz="0" iyy="2" iyz="0" izz="3"/></inertial></link>
  <link name="sensor"/>
  <joint name="sj" type="fixed"><parent link="b"/><child link="sensor"/><origin xyz="0 0 0.1"/></joint>
  <joint name="j2" type="revolute"><origin xyz="0 0 1"/><axis xyz="0 1 0.5"/><parent link="a"/><child link="b"/>
     <limit effort="1" lower="-1" upper="2" velocity="3"/><dynamics damping="0.7" friction="0.2"/></joint>
  <link name="b"><inertial><mass value="1"/><inertia ixx="0.1" ixy="0" ixz="0" iyy="0.1" iyz="0" izz="0.1"/></inertial></link>
  <joint name="j1" type="continuous"><parent link="a"/><child link="c"/></joint>
  <link name="c"><inertial><mass value="0.5"/><inertia ixx="0.1" ixy="0" ixz="0" iyy="0.1" iyz="0" izz="0.1"/></inertial></link>
</robot>"""


def test_parse_rules(tmp_path):
    p = tmp_path / "t.urdf"
    p.write_text(_URDF)
    # default serialisation = iDynTree's walk: the child whose joint comes LAST in the document is visited first
    tt = parse_urdf(str(p))
    assert tt.link_names == ["a", "c", "b"] and tt.parent == [-1, 0, 0]
    assert tt.dof_names == ["j1", "j2"] and tt.dof_index == [-1, 0, 1]
    assert tt.frames["sensor"]["link"] == 2 and tt.frames["world_box"]["link"] == 0
    assert np.array_equal(tt.params[1], parse_urdf(str(p), link_order="document").params[2])
    # explicit lists win; JSON round trip keeps the document ranks, so either order can be rebuilt from a stored topology
    t4 = parse_urdf(str(p), link_names=["b", "a", "c"], joint_names=["j2", "j1"])
    assert t4.link_names == ["b", "a", "c"] and t4.parent == [1, -1, 1] and t4.dof_index == [0, -1, 1] and t4.frames["sensor"]["link"] == 0
    back = Topology.from_dict(json.loads(json.dumps(t4.to_dict()))).serialized("traversal", "traversal")
    assert back.link_names == tt.link_names and back.dof_names == tt.dof_names and back.dof_index == tt.dof_index
    with pytest.raises(ValueError):
        parse_urdf(str(p), link_names=["a", "b"])
    t = parse_urdf(str(p), link_order="document", dof_order="document")
    # fake root and fake leaf removed, document order kept, DOFs in document order of the movable joints
    assert t.link_names == ["a", "b", "c"]
    assert t.parent == [-1, 0, 0]
    assert t.dof_names == ["j2", "j1"] and t.dof_index == [-1, 0, 1]
    assert set(t.frames) == {"world_box", "sensor"} and t.frames["sensor"]["link"] == 1
    assert np.allclose(np.linalg.norm(t.axis[1]), 1.0) and np.allclose(t.axis[1], np.array([0, 1, 0.5]) / np.sqrt(1.25))
    assert np.allclose(t.axis[2], [1, 0, 0])  # URDF default axis
    # inertial origin rpy rotates the inertia (90 deg about z swaps xx/yy), parallel axis to the link origin
    assert np.allclose(t.params[0], [2, 0.2, 0, 0, 2, 0, 0, 1 + 2 * 0.01, 0, 3 + 2 * 0.01])
    assert t.limits["j2"] == {"torque": 1.0, "lower": -1.0, "upper": 2.0, "velocity": 3.0}
    assert "j1" not in t.limits  # only 'revolute' joints carry limits in the reference (helpers.py:907)
    assert t.friction["j2"] == {"f_constant": 0.2, "f_velocity": 0.7}
    # first <origin> wins; the fake root frame is the inverse of the joint origin
    f = t.frames["world_box"]
    assert f["link"] == 0 and np.allclose(f["R"] @ np.array([1, 2, 3.0]) + f["p"], 0)
    t2 = Topology.from_dict(json.loads(json.dumps(t.to_dict())))
    assert t2.link_names == t.link_names and np.array_equal(t2.params, t.params)
    t3 = t.reordered_dofs(["j1", "j2"])
    assert t3.dof_index == [-1, 1, 0]


def test_kuka_apriori_vector_matches_tutorial_table():
    """F9: documentation/TUTORIAL.md:60-160 prints xStdModel[0:101] to 8 decimals."""
    g = json.load(open(os.path.join(GOLDEN, "kuka_tutorial_apriori.json")))
    t = load_topo("kuka_lwr4")
    x = t.x_std()
    ref = np.array(g["xStdModel"])
    assert x.shape == (80,)
    assert np.abs(x - ref[:80]).max() <= 5.0e-9
    fc = [t.friction[j]["f_constant"] for j in t.dof_names]
    fv = [t.friction[j]["f_velocity"] for j in t.dof_names]
    assert np.allclose(fc, ref[80:87]) and np.allclose(fv, ref[87:94]) and np.all(ref[94:] == 0)
    assert t.link_names == ["lwr_base_link"] + [f"lwr_{i}_link" for i in range(1, 8)]
    assert t.dof_names == [f"lwr_{i}_joint" for i in range(7)]
    assert abs(t.params[:, 0].sum() - g["apriori_mass"]) < 1e-12


def test_default_serialisation_reproduces_the_reference_held_joint_lists():
    """model/*_regressor.xml list the joints 'in the same order as reported when running without supplying a regressor file'
    (walkman_regressor.xml:1), i.e. iDynTree's DOF serialisation (model.py:86-94); configs/walkman_static.yaml:60-64 repeats
    the WALK-MAN list.  The default topology must reproduce them; URDF document order does not (WALK-MAN)."""
    g = json.load(open(os.path.join(GOLDEN, "reference_joint_orders.json")))
    for name in ("threeLinks", "kuka_lwr4", "walkman_left_arm", "walkman_apriori"):
        t = load_topo(name)
        assert t.dof_names == g[name], name
        assert t.dof_order("traversal") == g[name]
        # links follow the same walk: every link is numbered after its parent, DOFs ascend along the link order
        assert all(t.parent[l] < l for l in range(t.num_links))
        d = [x for x in t.dof_index if x >= 0]
        assert d == sorted(d)
        u = parse_urdf(os.path.join(URDF_DIR, name + ".urdf"))
        assert u.link_names == t.link_names and u.dof_names == t.dof_names and u.parent == t.parent
    w = load_topo("walkman_apriori")
    assert w.dof_names == g["walkman_static_yaml"]
    assert w.dof_order("document") != g["walkman_apriori"] and w.dof_order("document")[:3] == ["WaistLat", "WaistSag", "WaistYaw"]
    assert w.link_names[:4] == ["Waist", "imu_link2", "imu_link", "LHipMot"] and w.link_names[-1] == "crane_ft"
    doc = w.serialized("document", "document")
    assert doc.link_names[:4] == ["Waist", "DWL", "DWS", "DWYTorso"]  # SURVEY.md Appendix A list
    assert sorted(doc.link_names) == sorted(w.link_names)
    # same physical robot: per-link parameters and frames follow their link
    for n in w.link_names:
        assert np.array_equal(w.params[w.link_names.index(n)], doc.params[doc.link_names.index(n)])
    for f in w.frames:
        assert w.link_names[w.frames[f]["link"]] == doc.link_names[doc.frames[f]["link"]]


def test_structure_counts():
    s = json.load(open(os.path.join(GOLDEN, "structure.json")))
    for name in ("threeLinks", "kuka_lwr4", "walkman_left_arm", "walkman_apriori"):
        t = load_topo(name)
        assert t.num_links == s[name]["links"] and t.num_dofs == s[name]["dofs"]
        order = t.traversal()
        pos = {l: i for i, l in enumerate(order)}
        assert all(t.parent[l] < 0 or pos[t.parent[l]] < pos[l] for l in range(t.num_links))
    w = load_topo("walkman_apriori")
    assert abs(w.params[:, 0].sum() - s["walkman_apriori"]["mass"]) < 0.01
    anc = w.ancestors_dofs()
    assert sum(len(a) for a in anc) == 228 and max(len(a) for a in anc) == 10


def test_urdf_write_back_round_trip(tmp_path):
    """replaceParamsInURDF (helpers.py:511-577): parameters written into a URDF copy and parsed again come back
    (link <-> barycentric conversions of helpers.py:374-435 are inverses; fake links / frames untouched)."""
    import os

    from flobaroid_amd import topology as T

    src = os.path.join(URDF_DIR, "kuka_lwr4.urdf")
    topo = T.parse_urdf(src)
    L = topo.num_links
    rng = np.random.default_rng(3)
    x = topo.x_std().copy()
    # perturb to a physically plausible set: scale masses, move COMs, add SPD inertia about the COM
    bary = T.params_link_to_bary(x, L)
    assert np.allclose(T.params_bary_to_link(bary, L), x, rtol=1e-12, atol=1e-14)
    for l in range(L):
        b = bary[10 * l:10 * l + 10]
        b[0] = b[0] * (1.0 + 0.2 * rng.random()) + 0.1
        b[1:4] += 0.01 * rng.standard_normal(3)
        A = rng.standard_normal((3, 3)) * 0.05
        Ic = A @ A.T + 0.01 * np.eye(3)
        b[4:10] = [Ic[0, 0], Ic[0, 1], Ic[0, 2], Ic[1, 1], Ic[1, 2], Ic[2, 2]]
    xnew = np.concatenate([T.params_bary_to_link(bary, L), 0.3 + rng.random(2 * topo.num_dofs)])
    out = str(tmp_path / "kuka_new.urdf")
    T.replace_params_in_urdf(src, out, topo, xnew, {"coulomb_offset": 10 * L, "viscous_offset": 10 * L + topo.num_dofs})
    t2 = T.parse_urdf(out)
    assert t2.link_names == topo.link_names and t2.dof_names == topo.dof_names
    assert np.allclose(t2.x_std(), xnew[: 10 * L], rtol=1e-12, atol=1e-13)
    for j, name in enumerate(topo.dof_names):
        assert abs(t2.friction[name]["f_constant"] - xnew[10 * L + j]) < 1e-14
        assert abs(t2.friction[name]["f_velocity"] - xnew[10 * L + topo.num_dofs + j]) < 1e-14


def test_prismatic_joints_are_parsed(tmp_path):
    """Any joint type with one DOF that iDynTree's loader takes (model.py:60-67): revolute / continuous / prismatic; limits of prismatic
    joints are read like those of revolute ones; multi-DOF joint types are refused by name."""
    from flobaroid_amd.topology import JOINT_PRISMATIC, JOINT_REVOLUTE

    urdf = """<robot name="slider">
      <link name="base"><inertial><mass value="1"/><inertia ixx="1" ixy="0" ixz="0" iyy="1" iyz="0" izz="1"/></inertial></link>
      <link name="cart"><inertial><mass value="2"/><origin xyz="0.1 0 0"/><inertia ixx="1" ixy="0" ixz="0" iyy="1" iyz="0" izz="1"/></inertial></link>
      <link name="arm"><inertial><mass value="3"/><inertia ixx="1" ixy="0" ixz="0" iyy="1" iyz="0" izz="1"/></inertial></link>
      <joint name="slide" type="prismatic"><parent link="base"/><child link="cart"/><origin xyz="0 0 0.5" rpy="0 0 0.3"/><axis xyz="0 2 0"/>
        <limit effort="10" lower="-0.4" upper="0.6" velocity="1.5"/><dynamics friction="0.1" damping="0.2"/></joint>
      <joint name="hinge" type="revolute"><parent link="cart"/><child link="arm"/><axis xyz="0 0 1"/><limit effort="5" lower="-1" upper="1" velocity="2"/></joint>
    </robot>"""
    p = tmp_path / "s.urdf"
    p.write_text(urdf)
    t = parse_urdf(str(p))
    l = t.link_names.index("cart")
    assert t.joint_type[l] == JOINT_PRISMATIC and t.joint_type[t.link_names.index("arm")] == JOINT_REVOLUTE and t.num_dofs == 2
    assert np.allclose(t.axis[l], [0, 1, 0]) and t.limits["slide"] == {"torque": 10.0, "lower": -0.4, "upper": 0.6, "velocity": 1.5}
    assert t.friction["slide"] == {"f_constant": 0.1, "f_velocity": 0.2}
    t2 = Topology.from_dict(json.loads(json.dumps(t.to_dict())))
    assert t2.joint_type == t.joint_type
    p.write_text(urdf.replace('type="prismatic"', 'type="planar"'))
    with pytest.raises(NotImplementedError, match="planar"):
        parse_urdf(str(p))
