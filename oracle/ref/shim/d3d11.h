// d3d11.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/). Plain structs under the Direct3D 11 names the
// reference's headers and its mesh / scene sources mention. The device and the context accept every call the
// mesh code makes and do nothing, so mesh::setup_mesh, bind and draw are no-ops.
#pragma once
#include "Windows.h"

enum DXGI_FORMAT {
    DXGI_FORMAT_UNKNOWN = 0,
    DXGI_FORMAT_R32G32B32_FLOAT = 6,
    DXGI_FORMAT_R32G32_FLOAT = 16,
    DXGI_FORMAT_R32_UINT = 42,
    DXGI_FORMAT_B8G8R8A8_UNORM = 87,
};
enum D3D11_INPUT_CLASSIFICATION { D3D11_INPUT_PER_VERTEX_DATA = 0, D3D11_INPUT_PER_INSTANCE_DATA = 1 };
enum D3D11_USAGE { D3D11_USAGE_DEFAULT = 0, D3D11_USAGE_IMMUTABLE = 1, D3D11_USAGE_DYNAMIC = 2, D3D11_USAGE_STAGING = 3 };
enum D3D11_BIND_FLAG {
    D3D11_BIND_VERTEX_BUFFER = 0x1,
    D3D11_BIND_INDEX_BUFFER = 0x2,
    D3D11_BIND_CONSTANT_BUFFER = 0x4,
    D3D11_BIND_SHADER_RESOURCE = 0x8,
};

struct D3D11_INPUT_ELEMENT_DESC {
    LPCSTR SemanticName;
    UINT SemanticIndex;
    DXGI_FORMAT Format;
    UINT InputSlot;
    UINT AlignedByteOffset;
    D3D11_INPUT_CLASSIFICATION InputSlotClass;
    UINT InstanceDataStepRate;
};
struct D3D11_BUFFER_DESC {
    UINT ByteWidth;
    D3D11_USAGE Usage;
    UINT BindFlags;
    UINT CPUAccessFlags;
    UINT MiscFlags;
    UINT StructureByteStride;
};
struct D3D11_SUBRESOURCE_DATA {
    const void* pSysMem;
    UINT SysMemPitch;
    UINT SysMemSlicePitch;
};
struct D3D11_MAPPED_SUBRESOURCE {
    void* pData;
    UINT RowPitch;
    UINT DepthPitch;
};

struct ID3D11Buffer {};
struct ID3D11RenderTargetView {};
struct ID3D11Texture2D {};
struct ID3D11ShaderResourceView {};
struct ID3D11SamplerState {};
struct ID3D11PixelShader {};
struct ID3D11VertexShader {};
struct ID3D11InputLayout {};
struct ID3D11RasterizerState {};
struct ID3D11DepthStencilState {};
struct ID3D11DepthStencilView {};
struct IDXGISwapChain {};
struct ID3DBlob {};
typedef ID3DBlob ID3D10Blob;

struct ID3D11Device {
    template <typename... A> HRESULT CreateBuffer(A&&...) { return S_OK; }
};
struct ID3D11DeviceContext {
    template <typename... A> void IASetVertexBuffers(A&&...) {}
    template <typename... A> void IASetIndexBuffer(A&&...) {}
    template <typename... A> void DrawIndexed(A&&...) {}
};
