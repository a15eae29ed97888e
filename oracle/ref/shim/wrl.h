// wrl.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/). A ComPtr that owns nothing: an empty one hands
// out one inert object per type, so calls through it are no-ops instead of null dereferences.
#pragma once

namespace Microsoft {
namespace WRL {

template <typename T>
class ComPtr {
public:
    ComPtr() = default;
    ComPtr(T* p) : m_ptr(p) {}
    T* Get() const { return m_ptr ? m_ptr : inert(); }
    T* operator->() const { return Get(); }
    T* const* GetAddressOf() const { return &m_ptr; }
    T** GetAddressOf() { return &m_ptr; }
    T** ReleaseAndGetAddressOf() { m_ptr = nullptr; return &m_ptr; }
    void Reset() { m_ptr = nullptr; }
    explicit operator bool() const { return m_ptr != nullptr; }

private:
    static T* inert() {
        static T object{};
        return &object;
    }
    T* m_ptr = nullptr;
};

}  // namespace WRL
}  // namespace Microsoft
