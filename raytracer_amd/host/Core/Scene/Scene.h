// Scene: owns the objects, builds the top-level BVH and flattens everything into the RtSceneDesc the
// device library uploads (reference: Core/Scene/Scene.h, Scene::BuildBVH Core/Scene/Scene.cpp:36-126).
#pragma once

#include "Object/SceneObject.h"
#include "../BVH/BVH.h"
#include "../../../../include/rtgpu.h"

namespace rt {

class RAYLIB_API Scene
{
public:
    Scene();
    ~Scene();
    Scene(Scene&&);
    Scene& operator=(Scene&&);

    void AddObject(SceneObjectPtr object);
    bool BuildBVH();

    // Moving objects (mirror-only; what the reference's demo does with ISceneObject::SetTransform and a second BuildBVH, Demo_UserInterface.cpp:659,701, minus
    // the re-flatten).  SetObjectTransform: the object of the index-th AddObject call.  UpdateBVH: rebuilds mTraceableObjectsBVH over the current boxes, reorders
    // mTraceableObjects and rewrites only the flat objects, the flat top nodes and the matrices of the flat lights; materials, meshes and textures keep the
    // numbering of the last BuildBVH (Flatten interns them in leaf order: a re-flatten after a reorder may renumber them).  Needs a BuildBVH before it.
    bool SetObjectTransform(uint32 index, const math::Matrix4& matrix);
    bool UpdateBVH();
    // what rtgpu_update_objects takes after UpdateBVH; previousIndex relates the leaf order to the one before that UpdateBVH
    void GetUpdate(RtSceneUpdate& out) const;
    uint64 GetUpdateId() const { return mUpdateId; }   // UpdateBVH calls since the last BuildBVH
    // Deforming meshes (mirror-only): MeshShape::UpdateVertices of the mesh the index-th AddObject call holds (numVertices must be the mesh's).  UpdateBVH then
    // rewrites that mesh's flat nodes, triangles and vertex shading in place -- GetDesc() is the refit scene -- and lists it for the device:
    // GetMeshUpdate(i) is what rtgpu_update_mesh takes for the i-th mesh the last UpdateBVH found changed, before that UpdateBVH's rtgpu_update_objects.
    bool SetMeshVertices(uint32 index, uint32 numVertices, const math::Float3* positions, const math::Float3* normals, const math::Float3* tangents);
    // Deforming meshes ON THE DEVICE (rtgpu_update_mesh_device): the mirror learns the new bounding box alone -- the refitted root's, as the call returned it.
    // SetMeshBounds sets the box of the mesh the index-th AddObject call holds; the next UpdateBVH builds the top level over it and counts every object over
    // the mesh as moved, WITHOUT listing the mesh in GetMeshUpdate (the device has its tables: the objects alone are sent).  The mesh is then device-owned
    // (MeshOnDevice): the mirror's positions, triangles and tree, and GetDesc()'s share of them, are stale until SetMeshVertices gives the mirror the word
    // again.  While any mesh is device-owned (AnyMeshOnDevice) BuildBVH refuses, and so does a renderer asked to upload the scene whole: either would
    // put the stale mesh back.
    bool SetMeshBounds(uint32 index, const math::Float3& min, const math::Float3& max);
    bool MeshOnDevice(uint32 index) const;
    bool AnyMeshOnDevice() const;
    // the flat mesh (GetDesc().meshes) the index-th AddObject call's mesh became at the last BuildBVH, and its vertex count: what rtgpu_update_mesh_device names
    bool GetObjectMesh(uint32 index, uint32* outMeshIndex, uint32* outNumVertices) const;
    ShapePtr GetObjectShape(uint32 index) const;   // the shape of the index-th AddObject call (null: a light, or no such object): a second object may share it (an instance)
    uint32 GetNumMeshUpdates() const { return (uint32)mDirtyMeshes.size(); }
    void GetMeshUpdate(uint32 i, RtMeshUpdate& out) const;
    bool ObjectsMovedInLastUpdate() const { return mObjectsMoved; }   // the last UpdateBVH changed a flat object, its place in the leaf order, or a light's matrices

    uint32 GetNumObjects() const { return (uint32)mAllObjects.size(); }
    const std::vector<const LightSceneObject*>& GetLights() const { return mLights; }
    const std::vector<const LightSceneObject*>& GetGlobalLights() const { return mGlobalLights; }
    const BVH& GetBVH() const { return mTraceableObjectsBVH; }

    // Flat, pointer-stable description of the scene as of the last BuildBVH().  Valid until the next
    // BuildBVH() or destruction.  blueNoise is filled in by the renderer (it is sampler data, not scene data).
    const RtSceneDesc& GetDesc() const { return mDesc; }
    uint64 GetBuildId() const { return mBuildId; }

private:
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    bool Flatten();

    std::vector<SceneObjectPtr> mAllObjects;
    std::vector<const ISceneObject*> mTraceableObjects;   // BVH leaf order after BuildBVH
    std::vector<const LightSceneObject*> mLights;
    std::vector<const LightSceneObject*> mGlobalLights;
    BVH mTraceableObjectsBVH;

    // flattened storage backing mDesc
    std::vector<RtNode> mFlatTopNodes, mFlatMeshNodes;
    std::vector<RtObject> mFlatObjects;
    std::vector<RtLight> mFlatLights;
    std::vector<uint32> mFlatGlobalLights;
    std::vector<RtMaterial> mFlatMaterials;
    std::vector<RtMesh> mFlatMeshes;
    std::vector<RtTriangle> mFlatTriangles;
    std::vector<RtVertexIndices> mFlatVertexIndices;
    std::vector<RtVertexShading> mFlatVertexShading;
    std::vector<RtTexture> mFlatTextures;
    std::vector<uint8> mFlatTexels;
    RtSceneDesc mDesc;
    uint64 mBuildId = 0;
    std::vector<uint32> mPreviousIndex;
    uint64 mUpdateId = 0;
    // per flat mesh its shape and the versions the flat arrays show; the flat meshes the last UpdateBVH rewrote (and whether their shading changed)
    struct FlatMesh { const class MeshShape* shape; uint64 version, shadingVersion, boundsVersion; };
    std::vector<FlatMesh> mFlatMeshShapes;
    std::vector<std::pair<uint32, bool>> mDirtyMeshes;
    bool mObjectsMoved = false;
};

} // namespace rt
