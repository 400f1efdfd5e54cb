// Shapes (host-side descriptions).  Mirrors the constructors of the reference's IShape family
// (Core/Shapes/*.h); intersection / sampling / frame evaluation run on the device.
#pragma once

#include "../Math/Math.h"
#include "../BVH/BVH.h"
#include "Mesh/VertexBufferDesc.h"

namespace rt {

class IShape
{
public:
    enum class Kind : uint32 { Sphere = 0, Box = 1, Rect = 2, Mesh = 3 };   // == RtShapeKind
    virtual ~IShape() = default;
    virtual Kind GetKind() const = 0;
    virtual const math::Box GetBoundingBox() const = 0;   // local space
    virtual float GetSurfaceArea() const { return 0.0f; }
    // shapeParam / shapeParam2 of RtObject / RtLight
    virtual void GetParams(float param[4], float param2[4]) const = 0;
};
using ShapePtr = std::shared_ptr<IShape>;

class RAYLIB_API SphereShape : public IShape
{
public:
    explicit SphereShape(const float radius);
    Kind GetKind() const override { return Kind::Sphere; }
    const math::Box GetBoundingBox() const override;
    float GetSurfaceArea() const override;
    void GetParams(float param[4], float param2[4]) const override;
private:
    float mRadius, mInvRadius;
};

class RAYLIB_API BoxShape : public IShape
{
public:
    explicit BoxShape(const math::Vector4& size);   // half extents
    Kind GetKind() const override { return Kind::Box; }
    const math::Box GetBoundingBox() const override;
    float GetSurfaceArea() const override;
    void GetParams(float param[4], float param2[4]) const override;
private:
    math::Vector4 mSize, mInvSize;
};

class RAYLIB_API RectShape : public IShape
{
public:
    explicit RectShape(const math::Float2 size = math::Float2(FLT_MAX), const math::Float2 texScale = math::Float2(1.0f));
    Kind GetKind() const override { return Kind::Rect; }
    const math::Box GetBoundingBox() const override;
    float GetSurfaceArea() const override;
    void GetParams(float param[4], float param2[4]) const override;
private:
    math::Float2 mSize, mTextureScale;
};

struct MeshDesc
{
    VertexBufferDesc vertexBufferDesc;
    std::string path;
};

// Triangle mesh with its own BVH.  Initialize() copies the borrowed arrays, builds the SAH BVH over the
// triangles and reorders them into BVH leaf order (reference: Core/Shapes/MeshShape.cpp:34-112,
// Core/Shapes/Mesh/VertexBuffer.cpp:52-186).
class RAYLIB_API MeshShape : public IShape
{
public:
    struct Triangle { float v0[3], edge1[3], edge2[3]; };                 // == RtTriangle
    struct VertexIndices { uint32 i0, i1, i2, materialIndex; };           // mesh-local material index
    struct VertexShading { float normal[3], tangent[3], texCoord[2]; };   // == RtVertexShading

    MeshShape();
    ~MeshShape() override;
    bool Initialize(const MeshDesc& desc);

    // Deforming (mirror-only; the device's half is rtgpu_update_mesh).  New positions -- and optionally normals and tangents -- for the SAME vertices, in the
    // order of the VertexBufferDesc the mesh was made from: the leaf order and the tree's topology stay, the triangles are recomputed with Initialize's
    // arithmetic and every node's box is refitted with Math.h's Box operations (a leaf: its triangles' boxes joined in order; an interior node: Box(child0,
    // child1)); the bounding box becomes the root's.  Scene::UpdateBVH picks the change up (GetVersion).
    bool UpdateVertices(const math::Float3* positions, const math::Float3* normals, const math::Float3* tangents);
    uint64 GetVersion() const { return mVersion; }                 // UpdateVertices calls so far
    uint64 GetShadingVersion() const { return mShadingVersion; }   // the last of them that brought normals or tangents
    const std::vector<math::Float3>& GetPositions() const { return mPositions; }   // of the last UpdateVertices (empty before the first)
    // The mesh was deformed ON THE DEVICE (rtgpu_update_mesh_device): only its new bounding box, the refitted root's, comes back.  The mesh is then
    // device-owned: positions, triangles and tree of the mirror no longer describe the device, until UpdateVertices gives the mirror the word again (and then
    // sends its normals and tangents too: the device's may be newer).  GetVersion stays: nothing is to be sent.
    void SetDeviceBounds(const math::Box& box) { mBoundingBox = box; mOnDevice = true; mBoundsVersion++; }
    bool IsOnDevice() const { return mOnDevice; }
    uint64 GetBoundsVersion() const { return mBoundsVersion; }     // SetDeviceBounds calls so far

    Kind GetKind() const override { return Kind::Mesh; }
    const math::Box GetBoundingBox() const override { return mBoundingBox; }
    void GetParams(float param[4], float param2[4]) const override;

    const BVH& GetBVH() const { return mBVH; }
    const std::vector<Triangle>& GetTriangles() const { return mTriangles; }
    const std::vector<VertexIndices>& GetVertexIndices() const { return mIndices; }
    const std::vector<VertexShading>& GetVertexShading() const { return mShading; }
    const std::vector<MaterialPtr>& GetMaterials() const { return mMaterials; }

private:
    BVH mBVH;
    math::Box mBoundingBox;
    std::vector<Triangle> mTriangles;
    std::vector<VertexIndices> mIndices;
    std::vector<VertexShading> mShading;
    std::vector<MaterialPtr> mMaterials;
    std::vector<math::Float3> mPositions;
    uint64 mVersion = 0, mShadingVersion = 0, mBoundsVersion = 0;
    bool mOnDevice = false;
};

using MeshShapePtr = std::shared_ptr<MeshShape>;

} // namespace rt
